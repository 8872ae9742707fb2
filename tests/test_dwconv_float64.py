"""Float64 checks of every form of the depthwise convolutions of csrc/conv.hip -- the 3 x 3 (+ bias, + GELU) strip kernels, vertical-walk
kernels, one-launch form of small maps, the Mix-FFN form that builds fc2's data gradient inside pass A, the deferred finalize, and the
7 x 7 kernels -- each against a plain float64 statement of the operation (tests/dwconv_refs.py) at the smallest shapes that reach each
path of the dispatch, and on inputs that are NOT friendly: a mean of 8 sigma under zero-sum weights, GELU saturated on both sides, the
linear region of gelu', a bias of -6, 80 % exact zeros with an all-zero image, a null bias.

Every bound is derived per element (dwconv_refs.py, module docstring): the fp32 multiply-add chain of the taps, the absolute error of the
kernels' erf (norm_refs.GELU_ERR) and of gelu_erf8<true> (dwconv_refs.GELU_GRAD_ERR), one rounding of the store.  Where a call leaves du in
memory, pass C and the weight / bias sums are held to what follows from the du that pass A WROTE; where it does not (the one-launch
form), to the float64 du plus the du bound carried through the taps.  dw / db: norm_refs' reduction class, max(2 e_ref, 4 * 2^-24 * scale).

Every GPU test forces its form with the existing switches (SEGFAC_DW_NO_WALK, SEGFAC_DW_WALK_ROWS, SEGFAC_DW_NO_SMALL,
SEGFAC_DW_SMALL_ALWAYS, SEGFAC_FFN_BWD_FUSED), asserts with hip.trace() that the kernels of that form and no kernel of another form ran,
and asserts segf_dwconv3x3_bwd_blocks against the plan restated in dwconv_refs.py.

Observed on an MI355X, the largest (err - half_ulp) / bound per (form, output) -- for dw / db the largest (err) / max(e_ref, FLOOR / MARGIN *
2^-24 * scale), allowed up to MARGIN = 2; the test fails above `allowed`:

    form                output     ratio  allowed  case
    ------------------  ------    ------  -------  ----
    dw3.fc2             db         0.104        2  fc2-1x70x36x256x64 bf16
    dw3.fc2             du         0.106        1  fc2-1x70x36x256x64 bf16
    dw3.fc2             dw         0.494        2  fc2-2x5x16x128x32 bf16
    dw3.fc2             dx        0.0968        1  fc2-1x70x36x256x64 bf16
    dw3.fc2.deferred    db         0.103        2  fc2-2x9x22x128x32 bf16
    dw3.fc2.deferred    du        0.0596        1  fc2-2x9x22x128x32 bf16
    dw3.fc2.deferred    dw         0.325        2  fc2-2x9x22x128x32 bf16
    dw3.fc2.deferred    dx             0        1  fc2-2x9x22x128x32 bf16
    dw3.small           db         0.891        2  dw3-plain-1x5x6x2056-id fp32
    dw3.small           dw          1.54        2  dw3-plain-1x5x6x2056-id fp32
    dw3.small           dx          0.99        1  dw3-sparse-2x9x22x640-gelu bf16
    dw3.small.deferred  db         0.158        2  dw3-plain-2x9x22x640-gelu bf16
    dw3.small.deferred  dw         0.344        2  dw3-plain-2x9x22x640-gelu bf16
    dw3.small.deferred  dx         0.938        1  dw3-plain-2x9x22x640-gelu bf16
    dw3.strip           db         0.877        2  dw3-offset-2x2x5x24-gelu fp32
    dw3.strip           du         0.404        1  dw3-tiny-2x9x22x640-gelu fp32
    dw3.strip           dw          1.53        2  dw3-sparse-2x9x22x640-gelu fp32
    dw3.strip           dx         0.538        1  dw3-negative-2x9x22x640-gelu fp32
    dw3.strip           y          0.481        1  dw3-plain-2x32x32x64-id fp32
    dw3.strip.deferred  db          0.25        2  dw3-plain-2x9x22x640-gelu fp32
    dw3.strip.deferred  du         0.354        1  dw3-plain-2x9x22x640-gelu fp32
    dw3.strip.deferred  dw         0.612        2  dw3-plain-2x9x22x640-gelu fp32
    dw3.strip.deferred  dx         0.403        1  dw3-plain-2x9x22x640-gelu fp32
    dw3.walk            db          1.28        2  dw3-plain-1x5x6x2056-gelu fp32
    dw3.walk            du         0.404        1  dw3-tiny-2x9x22x640-gelu fp32
    dw3.walk            dw          1.61        2  dw3-plain-1x5x6x2056-gelu fp32
    dw3.walk            dx         0.538        1  dw3-negative-2x9x22x640-gelu fp32
    dw3.walk            y          0.481        1  dw3-plain-2x32x32x64-id fp32
    dw3.walk.deferred   db          0.25        2  dw3-plain-2x9x22x640-gelu fp32
    dw3.walk.deferred   du         0.354        1  dw3-plain-2x9x22x640-gelu fp32
    dw3.walk.deferred   dw         0.492        2  dw3-plain-2x9x22x640-gelu bf16
    dw3.walk.deferred   dx         0.403        1  dw3-plain-2x9x22x640-gelu fp32
    dw7                 db         0.633        2  dw7-nobias-2x9x11x2816 fp32
    dw7                 dw          1.09        2  dw7-nobias-1x9x17x96 fp32
    dw7                 dx         0.106        1  dw7-plain-2x9x11x2816 fp32
    dw7                 y            0.1        1  dw7-plain-2x9x11x2816 fp32

(dx of the one-launch form in bf16 comes close to 1 by construction: the bound's largest share is du's rounding to bf16 in LDS, |w| times
half a unit of du per tap, and where few taps are live -- a sparse map -- that share is reached whenever du lies next to a tie.)

The DERIVED terms, each with its derivation in dwconv_refs.py (where `DERIVED` is read), and the cases they apply to:
  GELU_CHAIN_TERM            y with GELU, every case: the roundings of the erf polynomial that norm_refs.GELU_ERR's count leaves out (the slope of
                             t p(t), intermediate values above 1) and the last multiply-add; the fp32 emulation on the CPU needs it
  UNDERFLOW                  t, y without GELU and dx, every case: one step of the denormal grid per multiply-add, where du underflows behind
                             a saturated GELU (class `big`)
  wgrad_roundings as floor   dw and db, class `negative` (b = -6): a handful of pixels carry a column's sum; the additions of the form's reduction
With dwconv_refs.DERIVED = False the issue's bound alone is applied; 4 of the 402 GPU cases are then outside it, none of them by a wrong
computation: dx of dw3-big-2x9x22x640-gelu in fp32 in the strip and walk forms (ratio 1.21: 6.4e-40 off by 4e-46, a third of a denormal
step), dw of dw3-negative-2x9x22x640-gelu in fp32 in the walk form (2.26 against 2) and in bf16 in the strip form (2.03 against 2).  CPU tests
show for each term that a plain fp32 computation needs it with no kernel involved (test_gelu_emulation_*, test_underflow_term_*,
test_another_order_of_the_fp32_sum_*).

Not covered: the block caps of the three weight-gradient plans (DWG_MAX_BLOCKS of the strip form, 2 * DWG_MAX_BLOCKS of the walk form, 256
of the 7 x 7), the walk kernel's own grid-stride loop, and walk segments longer than a policy-forced 64 rows under the default policy: all
need tens of millions of elements.  The second iteration of dwconv7x7_kernel's strip loop is reached by the sampled 67 M-element case of
tests/test_exact_kernels.py.
"""
import pytest
import torch
import torch.nn.functional as F

import dwconv_refs as D
import exact_inputs as X
import norm_refs as R

BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
DT_ID = {F32: 'fp32', BF: 'bf16'}
gpu = pytest.mark.gpu
CASES3, CASES7 = D.cases3(), D.cases7()


def _settle(op, Y, verdicts):
    """Print every figure, then assert."""
    for name, v in verdicts.items():
        print(f'RATIO {op} {name} {Y.case["id"]} {DT_ID[Y.dtype]} {v.ratio:.4g}')
    bad = [v.message for v in verdicts.values() if not v.ok]
    assert not bad, '\n'.join(bad)


# ---- CPU: the references against autograd ---------------------------------------------------------------------------------------------
def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize('gelu', [True, False])
@pytest.mark.parametrize('k,shape', [(3, (2, 5, 7, 6)), (3, (2, 1, 6, 4)), (3, (2, 6, 1, 4)), (3, (1, 1, 1, 3)), (3, (1, 2, 2, 3)),
                                     (7, (2, 9, 11, 5)), (7, (2, 1, 9, 4)), (7, (2, 8, 1, 4)), (7, (1, 1, 1, 3)), (7, (2, 3, 5, 4))])
def test_reference_agrees_with_autograd(k, shape, gelu):
    """The slice sums against float64 autograd of F.conv2d(groups = C) + F.gelu to 1e-12: H = 1, W = 1, one pixel, maps smaller than the kernel."""
    B, H, W, C = shape
    g = X.gen(k * 100 + H * 10 + W)
    x, dy = (torch.randn(B, H, W, C, generator=g, dtype=torch.float64) for _ in range(2))
    w, b = 0.3 * torch.randn(C, k * k, generator=g), torch.randn(C, generator=g)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr, br = w.double().reshape(C, 1, k, k).requires_grad_(True), b.double().requires_grad_(True)
    t = F.conv2d(xr, wr, br, padding=k // 2, groups=C)
    tl = t.detach().requires_grad_(True)
    y = F.gelu(tl) if gelu else tl * 1.0
    y.backward(dy.permute(0, 3, 1, 2))
    t.backward(tl.grad)
    back = lambda v: v.permute(0, 2, 3, 1)                      # noqa: E731
    f = D.fwd_ref(x, w, b, k, gelu)
    du = D.du_ref(f['t'], dy, gelu)
    dx, A_dx = D.dx_ref(du, w, k)
    dw, db, s_dw, s_db = D.wgrad_ref(x, du, k)
    assert _rel(f['y'], back(y.detach())) <= 1e-12 and _rel(du, back(tl.grad)) <= 1e-12 and _rel(dx, back(xr.grad)) <= 1e-12
    assert _rel(dw, wr.grad.reshape(C, k * k)) <= 1e-12 and _rel(db, br.grad) <= 1e-12
    # the absolute sums are those of the same terms
    assert (f['A_t'] >= f['t'].abs() * (1 - 1e-12)).all() and (A_dx >= dx.abs() * (1 - 1e-12)).all()
    assert (s_dw >= dw.abs() * (1 - 1e-12)).all() and (s_db >= db.abs() * (1 - 1e-12)).all()
    xa, wa = x.abs(), w.abs()
    assert _rel(f['A_t'], D.fwd_ref(xa, wa, b.abs(), k, False)['t']) <= 1e-12


def test_gelu_constants():
    x = torch.linspace(-8, 8, 1 << 16, dtype=torch.float64)
    g1 = R.gelu_grad64(x)
    g2 = (2 - x * x) * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5
    assert g1.abs().max() <= D.G1 and D.G1 - g1.abs().max() < 1e-6
    assert g2.abs().max() <= D.G2 + 1e-15 and D.G2 - g2.abs().max() < 1e-6
    assert D.GELU_GRAD_ERR < 7e-7 and D.GELU_ERR + D.GELU_CHAIN_TERM < 4e-7


def test_gelu_emulation_stays_inside_both_constants():
    """gelu_erf8 of csrc/common.h evaluated operation for operation in torch fp32, on a dense grid over [-12, 12] and at the tiny and huge
    ends, against gelu64 / gelu_grad64: |d gelu'| <= GELU_GRAD_ERR, and |d gelu| <= (GELU_ERR + GELU_CHAIN_TERM) |x|.  GELU_ERR alone is NOT
    enough, with no kernel involved: its count of the erf roundings is short (dwconv_refs.ERF_ROUNDINGS), and the emulation is at 1.44 times
    GELU_ERR |x| near |x| = 0.06 -- the reason for the DERIVED term of y.  The constants are derived, not fitted: the shares are printed."""
    grid = torch.linspace(-12, 12, (1 << 21) + 1, dtype=torch.float64)
    ends = torch.tensor([s * m * 2.0 ** e for s in (-1, 1) for m in (1.0, 1.37) for e in list(range(-40, -3)) + list(range(4, 40))],
                        dtype=torch.float64)
    x32 = torch.cat([grid, ends, torch.zeros(1, dtype=torch.float64)]).float()
    x = x32.double()
    ey = (D.gelu_erf8_emulated(x32, False).double() - R.gelu64(x)).abs()
    eg = (D.gelu_erf8_emulated(x32, True).double() - R.gelu_grad64(x)).abs()
    plain = (ey / (D.GELU_ERR * x.abs()).clamp_min(1e-300)).max().item()
    print(f'gelu: largest error / (GELU_ERR |x|) = {plain:.3f}, / ((GELU_ERR + GELU_CHAIN_TERM) |x|) = '
          f'{(ey / ((D.GELU_ERR + D.GELU_CHAIN_TERM) * x.abs()).clamp_min(1e-300)).max().item():.3f}; '
          f"gelu': largest error / GELU_GRAD_ERR = {(eg / D.GELU_GRAD_ERR).max().item():.3f}")
    assert torch.isfinite(ey).all() and torch.isfinite(eg).all()
    assert (ey <= (D.GELU_ERR + D.GELU_CHAIN_TERM) * x.abs()).all()
    assert (eg <= D.GELU_GRAD_ERR).all()
    assert 1.0 < plain < 1.5
    # the slope of P(t) = t p(t) that the derivation uses
    t = torch.linspace(0, 1, 100001, dtype=torch.float64)
    slope = 5 * 1.061405429 * t ** 4 - 4 * 1.453152027 * t ** 3 + 3 * 1.421413741 * t ** 2 - 2 * 0.284496736 * t + 0.254829592
    assert slope.abs().max() <= 3.444 + 1e-3


# ---- CPU: the tables, the fp32 statement, the mutants ---------------------------------------------------------------------------------
def test_case_tables_are_well_formed():
    ids = [c['id'] for c in CASES3 + CASES7]
    assert len(set(ids)) == len(ids)
    assert {c['shape'] for c in CASES3 if c['cls'] == 'plain'} == {s for s, _ in D.SHAPES3}
    assert {(c['shape'], c['cls']) for c in CASES3 if c['cls'] != 'plain'} == {(s, k) for s in D.CLASS_SHAPES for k in D.CLASSES[1:]}
    assert {c['shape'] for c in CASES7 if c['cls'] in ('plain', 'nobias')} == {s for s, _ in D.SHAPES7}
    # what the shapes are there to reach (host arithmetic restated in dwconv_refs.py; test_host_plans_* holds it to the library)
    sm = lambda dt, s: D.small_nch(dt, *s, always=True)        # noqa: E731
    assert not sm(BF, (2, 3, 5, 40)) and sm(BF, (2, 4, 4, 40)) and sm(F32, (2, 16, 32, 64)) and not sm(F32, (2, 32, 32, 64))
    assert sm(BF, (2, 32, 32, 64)) and not sm(BF, (1, 33, 32, 64))
    assert (sm(BF, (2, 9, 22, 640)), sm(F32, (2, 9, 22, 640))) == (4, 2)
    assert D.walk_plan(1, 70, 6, 136) == (5, 16) and D.walk_plan(2, 130, 7, 16, 3) == (3, 44) and D.walk_plan(2, 2, 5, 24)[0] < 3
    assert D.dw7_strips_per_thread(8, 128, 128, 512) == 2 and all(D.dw7_strips_per_thread(*s) == 1 for s, _ in D.SHAPES7)
    # what the classes promise
    i = D.inputs(D.CASE_BY_ID['dw3-sparse-2x9x22x640-gelu'], BF)
    assert not i['x'][-1].any() and not i['dy'][-1].any() and 0.75 < (i['x'][0] == 0).double().mean() < 0.85
    i = D.inputs(D.CASE_BY_ID['dw3-offset-2x9x22x640-gelu'], F32)
    f = D.fwd_ref(i['x'], i['w'], i['b'], 3, True)
    assert (f['A_t'][:, 1:-1, 1:-1] / (f['t'][:, 1:-1, 1:-1].abs() + 1)).median() > 3
    assert D.inputs(D.CASE_BY_ID['dw3-nobias-2x2x5x24-gelu'], F32)['b'] is None
    i = D.inputs(D.CASE_BY_ID['dw3-big-2x9x22x640-gelu'], F32)
    t = D.fwd_ref(i['x'], i['w'], i['b'], 3, True)['t']
    assert (t > 8).double().mean() > 0.3 and (t < -8).double().mean() > 0.3
    i = D.inputs(D.CASE_BY_ID['dw3-tiny-2x9x22x640-gelu'], F32)
    assert D.fwd_ref(i['x'], i['w'], i['b'], 3, True)['t'].abs().max() < 2e-3
    for shape, rows in D.FC2_CASES:
        i = D.fc2_inputs(shape, rows)
        assert torch.equal(i['dy'].reshape(-1, shape[3]), X.round_bf16(i['dys'] @ i['w2']).double())


def _both(Y, got):
    """The verdicts of one set of outputs judged both ways: with du in memory (the tight check) and without."""
    v = {f'{k}': w for k, w in D.judge(Y, got).items()}
    v.update({f'{k} (no du)': w for k, w in D.judge(Y, {k: t for k, t in got.items() if k != 'du'}, only=('dx', 'dw', 'db')).items()})
    return v


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.values())
@pytest.mark.parametrize('case', CASES3 + CASES7, ids=lambda c: c['id'])
def test_plain_fp32_statement_is_inside_every_bound(case, dtype):
    """F.conv2d and F.gelu in fp32 on the CPU with autograd, no kernel involved: the reference alone must pass its own bar on every case."""
    Y = D.yard(case, dtype)
    v = _both(Y, D.statement32(Y))
    for name, w in v.items():
        print(f'RATIO cpu-fp32 {name} {case["id"]} {DT_ID[dtype]} {w.ratio:.4g}')
    bad = [w.message for w in v.values() if not w.ok]
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', list(D.MUTANTS))
def test_every_mutant_fails_the_comparison_the_gpu_tests_use(name):
    """Each wrong computation, applied to the float64 statement on the GPU tests' own inputs and rounded to the storage type, is rejected on
    at least one case of each dtype -- by outputs on which the unmutated statement of the same inputs is accepted."""
    selectors, outputs, bf_only = D.MUTANTS[name]
    chosen = [c for c in CASES3 + CASES7 if c['id'] in selectors]
    assert len(chosen) == len(selectors), (name, selectors)
    for dtype in ([BF] if bf_only else DTYPES):
        rejected = []
        for case in chosen:
            Y = D.yard(case, dtype)
            clean = D.statement64(Y)
            mutant = D.statement64(Y, name)
            for ways in (lambda g: g, lambda g: {k: t for k, t in g.items() if k != 'du'}):
                v = D.judge(Y, ways(clean), only=outputs)
                if not v:                                      # (du is the only output that may reject it, and this way has none)
                    continue
                assert all(v.values()), (name, case['id'], [w.message for w in v.values() if not w.ok])
                if not all(D.judge(Y, ways(mutant), only=outputs).values()):
                    rejected.append(case['id'])
        assert rejected, f'{name} passes in {DT_ID[dtype]} on {[c["id"] for c in chosen]}'


def test_another_order_of_the_fp32_sum_needs_the_negative_floor(monkeypatch):
    """The reason for the DERIVED floor of dw in the class `negative`, without any kernel: the plain sequential fp32 sum of the same fp32
    terms, taken over the pixels in another (fixed) order, is outside max(2 e_ref, 4 * 2^-24 * scale) -- e_ref is ONE sample of an order's
    error per column -- and inside the floor that counts the additions of a form's reduction."""
    case = D.CASE_BY_ID['dw3-negative-2x9x22x640-gelu']
    Y = D.yard(case, F32)
    st = D.statement64(Y)
    sh = D.Shifted(Y.inp['x'], 3)
    perm = torch.randperm(2 * 9 * 22, generator=X.gen(5))
    dw = torch.stack([R.seq_sum32((st['du'].double() * sh(ky, kx)).reshape(-1, 640).float()[perm]) for ky, kx in D.taps(3)], 1)
    got = dict(du=st['du'], dw=dw)
    v = D.judge(Y, got, only=('dw',))['dw']
    assert not v.ok and v.ratio > 4, v.ratio
    floors = [D.wgrad_roundings(form, F32, *case['shape']) for form in ('strip', 'walk', 'small')]
    assert floors == [36, 45, 46], floors
    for form in ('strip', 'walk', 'small'):
        assert D.judge(Y, got, only=('dw',), form=form)['dw'].ok
    monkeypatch.setattr(D, 'DERIVED', False)
    assert not D.judge(Y, got, only=('dw',), form='walk')['dw'].ok


def test_underflow_term_is_one_denormal_step_per_tap():
    """The reason for dwconv_refs.UNDERFLOW, without any kernel: a sum of denormal products rounded to fp32 misses the relative bound."""
    du = torch.full((1, 1, 1, 8), 2.0 ** -140, dtype=torch.float64)
    w = torch.full((8, 9), 0.3)
    dx, A = D.dx_ref(du, w, 3)
    err = (dx.float().double() - dx).abs().max().item()
    assert 9 * R.U24 * A.max().item() < err <= D.UNDERFLOW


def test_host_plans_restated_in_the_references_are_the_library_s(monkeypatch):
    """segf_dwconv3x3_bwd_blocks and the kernels a dry run names, for every 3 x 3 case in every form, against dwconv_refs' restatement of
    dw_small_nch, dw_walk_plan, dwg_plan and dww_plan (host arithmetic only: no GPU)."""
    from segmentation_factory_amd import hip
    L = hip.lib()
    for case in CASES3:
        if case['cls'] != 'plain' or not case['gelu']:
            continue
        for dtype in DTYPES:
            for form, rows in D.forms3(case, dtype, backward=True):
                _force(monkeypatch, form, rows)
                assert L.segf_dwconv3x3_bwd_blocks(hip.dt_of(torch.empty(0, dtype=dtype)), *case['shape']) == D.wgrad_blocks(form, dtype, *case['shape'], rows)
                with hip.trace(dry_run=True) as t:
                    assert L.segf_dwconv3x3_gelu_bwd(hip.dt_of(torch.empty(0, dtype=dtype)), *case['shape'], 16, 16, 16, 1, 16, 16, 16, 16, 16, 16, None) == 0
                _ran(t, form, dtype, True)
    _release(monkeypatch)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hip():
    from segmentation_factory_amd import hip
    hip.lib()
    return hip


_release, _force, _ran = D.release_forms, D.force_form, D.assert_form_ran


def _dev(t, dtype=F32):
    """A CPU tensor (float64 activations are already rounded to `dtype`: the cast is exact) as [rows][C] on the device."""
    return None if t is None else t.reshape(-1, t.shape[-1]).to(dtype).cuda().contiguous() if t.dim() > 1 else t.to(dtype).cuda().contiguous()


def _cpu(t):
    return None if t is None else t.detach().cpu()


def _form_params(cases, backward):
    return [pytest.param(c, dt, form, rows, id=f'{c["id"]}-{DT_ID[dt]}-{form}{f"-rows{rows}" if rows else ""}')
            for c in cases for dt in DTYPES for form, rows in D.forms3(c, dt, backward)]


def _raw_bwd(hip, x, w, b, dy, shape, gelu, keep_du, defer=False):
    """segf_dwconv3x3_gelu_bwd itself, so that the du of the three-pass forms can be read back.  -> dict(du, dx, dw, db)."""
    B, H, W, C = shape
    du = torch.full_like(x, float('nan'))
    dx = torch.empty_like(x)
    flat = torch.zeros(10 * C, dtype=F32, device=x.device)
    dw, db = flat[:9 * C].view(C, 9), flat[9 * C:]
    ws = torch.empty(int(hip.lib().segf_dwconv3x3_bwd_ws(B, H, W, C)), dtype=F32, device=x.device)
    rc = hip.lib().segf_dwconv3x3_gelu_bwd(hip.dt_of(x), B, H, W, C, x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), int(gelu),
                                           dy.data_ptr(), du.data_ptr(), dx.data_ptr(), None if defer else dw.data_ptr(),
                                           None if defer else db.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    if defer:
        hip.colreduce_finalize_grouped([(ws, int(hip.lib().segf_dwconv3x3_bwd_blocks(hip.dt_of(x), B, H, W, C)), 10 * C, dw, C)])
    torch.cuda.synchronize()
    return dict(du=_cpu(du) if keep_du else None, dx=_cpu(dx), dw=_cpu(dw), db=_cpu(db))


@gpu
@pytest.mark.parametrize('case,dtype,form,rows', _form_params(CASES3, False))
def test_dwconv3x3_forward(hip, case, dtype, form, rows, monkeypatch):
    Y = D.yard(case, dtype)
    i, (B, H, W, C) = Y.inp, case['shape']
    _force(monkeypatch, form, rows)
    with hip.trace() as t:
        y = hip.dwconv3x3_gelu_fwd(_dev(i['x'], dtype), _dev(i['w']), _dev(i['b']), B, H, W, C, case['gelu'])
    torch.cuda.synchronize()
    _ran(t, form, dtype, False)
    _settle(f'dw3.{form}', Y, D.judge(Y, dict(y=_cpu(y))))


@gpu
@pytest.mark.parametrize('case,dtype,form,rows', _form_params(CASES3, True))
def test_dwconv3x3_backward(hip, case, dtype, form, rows, monkeypatch):
    """du, dx, dw, db of segf_dwconv3x3_gelu_bwd in one forced form with the direct finalize; the three-pass forms leave du in memory."""
    Y = D.yard(case, dtype)
    i, shape = Y.inp, case['shape']
    _force(monkeypatch, form, rows)
    assert hip.lib().segf_dwconv3x3_bwd_blocks(hip.dt_of(torch.empty(0, dtype=dtype)), *shape) == D.wgrad_blocks(form, dtype, *shape, rows)
    with hip.trace() as t:
        got = _raw_bwd(hip, _dev(i['x'], dtype), _dev(i['w']), _dev(i['b']), _dev(i['dy'], dtype), shape, case['gelu'], keep_du=form != 'small')
    _ran(t, form, dtype, True)
    _settle(f'dw3.{form}', Y, D.judge(Y, got, form=form, rows=rows))


@gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.values())
@pytest.mark.parametrize('form', ['strip', 'walk', 'small'])
def test_dwconv3x3_backward_deferred_finalize(hip, form, dtype, monkeypatch):
    """Once per form: the partial sums left in the workspace and finalized by segf_colreduce_finalize_grouped afterwards."""
    case = D.CASE_BY_ID['dw3-plain-2x9x22x640-gelu']
    Y = D.yard(case, dtype)
    i, shape = Y.inp, case['shape']
    _force(monkeypatch, form)
    assert hip.lib().segf_dwconv3x3_bwd_blocks(hip.dt_of(torch.empty(0, dtype=dtype)), *shape) == D.wgrad_blocks(form, dtype, *shape)
    with hip.trace() as t:
        got = _raw_bwd(hip, _dev(i['x'], dtype), _dev(i['w']), _dev(i['b']), _dev(i['dy'], dtype), shape, True, keep_du=form != 'small', defer=True)
    assert any('colreduce_finalize' in k for k in t.kernels) and not any('dw_scatter_kernel' in k for k in t.kernels), t.kernels
    _settle(f'dw3.{form}.deferred', Y, D.judge(Y, got, form=form))


@gpu
@pytest.mark.parametrize('shape,rows,defer', [(s, r, False) for s, r in D.FC2_CASES] + [D.FC2_CASES[1] + (True,)],
                         ids=[f'{D._sid(s)}{f"-rows{r}" if r else ""}' for s, r in D.FC2_CASES] + ['deferred'])
def test_dwconv3x3_fc2_form(hip, shape, rows, defer, monkeypatch):
    """The Mix-FFN form (bf16) held to float64 itself, not only to the two launches it replaces: dys and w2 are lattice values, so the
    gradient rows dg = dys W2 that never exist in memory are exact integers with ONE known rounding to bf16.  The deferred finalize runs once."""
    B, H, W, Cc, Cin = shape
    case = dict(id=f'fc2-{D._sid(shape)}{f"-rows{rows}" if rows else ""}', k=3, shape=(B, H, W, Cc), cls='fc2', gelu=True)
    i = D.fc2_inputs(shape, rows)
    Y = D.make_yard(case, i, BF)
    _force(monkeypatch, 'walk', rows, fused=2)
    assert hip.dwconv3x3_gelu_bwd_fc2_supported(BF, B, H, W, Cc, Cin)
    assert hip.lib().segf_dwconv3x3_bwd_blocks(hip.BF16, B, H, W, Cc) == D.wgrad_blocks('walk', BF, B, H, W, Cc, rows)
    args = (_dev(i['x'], BF), _dev(i['w']), _dev(i['b']), _dev(i['dys'], BF), _dev(i['w2'], BF), B, H, W, Cc, Cin)
    with hip.trace() as t:
        if defer:
            flat = torch.zeros(10 * Cc, dtype=F32, device='cuda')
            dw, db = flat[:9 * Cc].view(Cc, 9), flat[9 * Cc:]
            dx, item, du = hip.dwconv3x3_gelu_bwd_fc2(*args, dw_out=dw, db_out=db, defer=True, return_du=True)
            hip.colreduce_finalize_grouped([item])
        else:
            dx, dw, db, du = hip.dwconv3x3_gelu_bwd_fc2(*args, return_du=True)
    torch.cuda.synchronize()
    want = [(f'dwconv3x3_walk_fc2_kernel<{Cin // 32}>',), ('dwconv3x3_wgrad_walk_kernel<T>',), ('dwconv3x3_walk_kernel<', 'MODE = 1]')]
    for subs in want:
        assert any(all(s in k for s in subs) for k in t.kernels), (subs, t.kernels)
    assert not any('MODE = 2]' in k or 'gemm' in k for k in t.kernels), t.kernels
    _settle('dw3.fc2' + ('.deferred' if defer else ''), Y, D.judge(Y, dict(du=_cpu(du), dx=_cpu(dx), dw=_cpu(dw), db=_cpu(db))))


@gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.values())
@pytest.mark.parametrize('case', CASES7, ids=lambda c: c['id'])
def test_dwconv7x7(hip, case, dtype):
    """Forward with and without bias; dx, dw, db; need_dx = False and need_db = False (the same sums, bit for bit, and no dx / db written)."""
    Y = D.yard(case, dtype)
    i, (B, H, W, C) = Y.inp, case['shape']
    x, dy, wt, b = _dev(i['x'], dtype), _dev(i['dy'], dtype), _dev(i['w'].t()), _dev(i['b'])
    with hip.trace() as t:
        y = hip.dwconv7x7_fwd(x, wt, b, B, H, W, C)
        dx, dw, db = hip.dwconv7x7_bwd(x, wt, dy, B, H, W, C)
    torch.cuda.synchronize()
    for n in ('dwconv7x7_kernel<T, false>', 'dwconv7x7_kernel<T, true>', 'dwconv7x7_wgrad_kernel<T>', 'dw7_scatter_kernel'):
        assert any(n in k for k in t.kernels), (n, t.kernels)
    with hip.trace() as t2:
        dx2, dw2, db2 = hip.dwconv7x7_bwd(x, wt, dy, B, H, W, C, need_dx=False, need_db=False)
    torch.cuda.synchronize()
    assert dx2 is None and db2 is None and not any('dwconv7x7_kernel' in k for k in t2.kernels), t2.kernels
    assert any('dwconv7x7_wgrad_kernel<T>' in k for k in t2.kernels) and torch.equal(dw2, dw)
    # the 7 x 7 has no activation: du IS dy, which is in memory, so dx / dw / db take the tight check
    got = dict(y=_cpu(y), du=i['dy'], dx=_cpu(dx), dw=_cpu(dw), db=_cpu(db))
    _settle('dw7', Y, {k: v for k, v in D.judge(Y, got).items() if k != 'du'})
