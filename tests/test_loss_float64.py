"""The fused upsample + CrossEntropy + Dice kernels (csrc/loss.hip, csrc/loss_band.hip) against the float64 statement of
tests/loss_refs.py: every dispatch path, class counts at the bucket edges, one-tap to 16 x 22 maps, row strides, and the inputs where
a softmax gradient goes wrong (confident pixels, constant logits, a large common offset, a spike on either side of the retry
threshold, absent classes, zero weights, ignored images).

Bound of every comparison (tests/loss_refs.py):  |got - ref64| <= half_ulp_T(ref64) + 4 * K * u * S  (+ the derived terms below).

MEASURED K (the reference statements' own error / (u S); CPU, every case of the tables, both storage types):
    stmt32 (u = 2^-24)         power-of-two ratios:  grad 85.1  I 126.1  P 58.8  ce_sum 2.09  w_sum 4.47  loss 15.1  log-sum 4.75
                               other ratios:         grad 37.1  I 12.5   P 4.78  ce_sum 1.04  w_sum 1.10  loss 14.2
    stmt_bf16tile (u = 2^-9)   grad 4.98   P 2.75
  (the confident inputs set them: a probability e^-30 carries the rounding of a difference of size 30.)  K is kept per output and per
  geometry class; each is at most the single largest one, which is what the bound is defined with.

DERIVED TERMS (all in tests/loss_refs.py, beside the formulas they come from):
  * every case, gradient / I / P: `under` -- an exponential below 2^-126 is flushed to zero in fp32 and bf16, so a probability has the
    absolute error 2^-126 exp(bound - log-sum); bound = the pixel's own maximum on the per-pixel and generic paths, the largest logit of
    the pixel's four taps on the batched ones (their wave-uniform stabiliser).
  * ce_sum (and loss): S counts 1 + |z_t - max| + |log-sum - z_t| per pixel instead of |log-sum - z_t| alone: the log of a sum >= 1
    that was rounded carries an absolute error 2^-24, whatever the difference that is left.
  * non-dyadic ratios (the `generic` rows), gradient / I / P / ce_sum / loss: `wobble` -- tap weights formed in fp32 carry an absolute
    error of WEIGHT_ROUNDINGS 2^-24 max(h, w), also where the exact weight is 0.
  * `_derived` below, terms of single paths found by the MI355X run: the bf16 staging of the full-resolution gradient on the generic
    path (gradient); log2(e) folded into the interpolation operand of the ratio-4 matrix-pipe kernels (ce_sum, loss); the stabiliser's
    size in the log-sum buffer (tests/loss_refs.py: lse_entry).

OBSERVED on the MI355X: the largest (|err| - half ulp) / (allowed error / 4) per path, storage type and output -- the number that must
stay at or below MARGIN = 4 -- in the table at the end of this docstring.

The path table is checked twice: on the CPU as dry runs through the C ABI with placeholder pointers (hip.ce_dice_fwd / ce_dice_bwd
allocate device tensors and ask for the current stream, so the wrappers themselves cannot run without a device; dispatch.replay_rc
makes the same calls), and in every GPU case with a live hip.trace() around the calls.

NOT COVERED: the argmax / confusion-matrix kernels of the same file; maps beyond 24 x 24 taps and 96 x 96 pixels (segment lengths
other than 8 and the default, grids of more than one round); B > 3; the `offset` inputs on non-dyadic ratios (the fp32 tap weights round
200 * 2^-24 into every logit there); labels outside [0, C) other than the ignore index; the `no_sets0_rule` mutant, which computes
the same function (test_sets0_rule_is_not_observable).

OBSERVED (MI355X; 546 GPU cases in 6.2 s; `-` = the path has no such output; 0 = bitwise the float64 value)
    generic    bfloat16  grad 3.2  I 1.1  P 1.2  ce_sum 1.4  w_sum 2.4  loss 0.044  lse -
    generic    float32   grad 0.69  I 0.9  P 1.2  ce_sum 1.4  w_sum 2.4  loss 0.038  lse -
    r1         bfloat16  grad 0.0063  I 0.17  P 0.22  ce_sum 1  w_sum 0.5  loss 0.061  lse -
    r1         float32   grad 0.75  I 0.26  P 0.26  ce_sum 1  w_sum 0.5  loss 0.061  lse -
    r2         bfloat16  grad 0.031  I 0.39  P 0.26  ce_sum 1.1  w_sum 0.73  loss 0.059  lse -
    r2         float32   grad 0.73  I 0.46  P 0.39  ce_sum 1.1  w_sum 0.73  loss 0.059  lse -
    r4         bfloat16  grad 0.63  I 1.9  P 0.98  ce_sum 0.89  w_sum 0.69  loss 0.44  lse 2.8
    r4         float32   grad 0.54  I 1.4  P 0.19  ce_sum 0.9  w_sum 0.69  loss 0.2  lse -
    r4_nolse   bfloat16  grad 0.39  I 2  P 0.47  ce_sum 0.76  w_sum 0  loss 0.44  lse -
    r4_nomfma  bfloat16  grad 4.4e-05  I 0.31  P 0.13  ce_sum 0.66  w_sum 0  loss 0.048  lse -
    r4_nomfma  float32   grad 0.36  I 0.44  P 0.15  ce_sum 0.65  w_sum 0  loss 0.048  lse -
    r4_rows8   bfloat16  grad 0.2  I 0.052  P 0.056  ce_sum 0.58  w_sum 0.3  loss 0.0094  lse 0.46
    r4_tile    bfloat16  grad 0.24  I 1.4  P 0.18  ce_sum 0.82  w_sum 0.7  loss 0.17  lse -
    r8         bfloat16  grad 0.012  I 0.22  P 0.16  ce_sum 2.7  w_sum 0.64  loss 0.14  lse -
    r8         float32   grad 0.19  I 0.14  P 0.24  ce_sum 2.7  w_sum 0.64  loss 0.14  lse -
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_refs as R                                                                     # noqa: E402

BF, F32, F64 = R.BF, R.F32, R.F64
CPU_CASES = R.cpu_cases()
GPU_CASES = R.gpu_cases()
_name = lambda dt: str(dt).replace('torch.', '')                                          # noqa: E731


def _ref(c, dtype, mut=None):
    inp = R.inputs(c, dtype)
    return inp, R.statement(inp['lo'], inp['t'], inp['cw'], c['go'], c['dice'], mut=mut)


def _is_tile(c, dtype):
    return dtype == BF and c['path'].startswith('r4')


def _entries(c, dtype, ref, derived=None):
    return R.entries(ref, dtype, R.geom_class(c), tile_fwd=R.band_covers(c, dtype), tile_bwd=_is_tile(c, dtype),
                     bound='exact' if c['path'] in ('r1', 'generic') else 'cell', derived=derived)


# ---- CPU: the statement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', (F32, BF), ids=_name)
def test_statement_agrees_with_float64_autograd(dtype):
    """Loss to 1e-12 relative, gradient to 1e-12 of its largest element, on every input class (and label kind, weight kind, ratio)."""
    from oracle import loss as OL
    for c in CPU_CASES:
        inp, ref = _ref(c, dtype)
        lr = inp['lo'].clone().requires_grad_(True)
        up = F.interpolate(lr, size=(c['H'], c['W']), mode='bilinear', align_corners=False)
        cw = None if inp['cw'] is None else inp['cw'].double()
        tot = OL.criterion_closed_form(up, inp['t'], cw, num_classes=c['C'], dice=c['dice'], ignore_index=R.IGNORE)
        (c['go'] * tot).backward()
        g = lr.grad.permute(0, 2, 3, 1).reshape(-1, c['C'])
        assert abs(tot.item() - ref['loss'][0].item()) <= 1e-12 * abs(tot.item()), c['id']
        assert (g - ref['grad']).abs().max().item() <= 1e-12 * g.abs().max().item(), c['id']
        assert abs(ref['loss'][0].item() - (ref['loss'][1] + ref['loss'][2]).item()) <= 1e-15 * abs(tot.item()), c['id']


def test_statement_agrees_with_the_loop_oracle():
    """criterion_loops (the reference's own batch x class loop; it builds its one-hot target in fp32, so it runs in fp32): the total
    inside the fp32 bound of the loss."""
    from oracle import loss as OL
    for c in (CPU_CASES[0], CPU_CASES[3], next(c for c in CPU_CASES if c['lab'] == 'image_ignored')):
        inp, ref = _ref(c, F32)
        up = F.interpolate(inp['lo'].float(), size=(c['H'], c['W']), mode='bilinear', align_corners=False)
        tot = OL.criterion_loops(up, inp['t'], inp['cw'], num_classes=c['C'], dice=c['dice'], ignore_index=R.IGNORE)
        en = R.entries(ref, F32, 'pow2', bound='exact')['loss']
        R.check(tot.reshape(1), en['ref'][:1], en['e'][:1], en['scale'][:1], F32, 'elementwise', c['id'], margin=R.MARGIN, floor=0.0)


def test_all_ignored_batch_statement_is_autograds():
    """No valid pixel in the batch: F.cross_entropy is 0 / 0 = NaN, and the gradient is ZERO, not NaN (an ignored pixel has no term)."""
    from oracle import loss as OL
    c = R.case('r4', 2, 19, 5, 6, 20, 24, lab='all_ignored')
    inp, ref = _ref(c, F32)
    lr = inp['lo'].clone().requires_grad_(True)
    up = F.interpolate(lr, size=(20, 24), mode='bilinear', align_corners=False)
    tot = OL.criterion_closed_form(up, inp['t'], None, num_classes=19, dice=True, ignore_index=R.IGNORE)
    tot.backward()
    assert math.isnan(tot.item()) and torch.isnan(ref['loss'][:2]).all() and ref['loss'][2].item() == 0.0
    assert not lr.grad.any() and not ref['grad'].any()


def test_log_sum_layout_round_trips():
    g = R.X.gen(3)
    for h, w in ((1, 1), (2, 3), (9, 10)):
        v = torch.randn(2, 4 * h, 4 * w, generator=g, dtype=F64)
        buf = R.lse_layout(v, h, w)
        assert buf.shape == (2, (h + 1) * (w + 1), 16) and torch.equal(R.lse_unlayout(buf, h, w), v)
        assert int(torch.isnan(buf).sum()) == 2 * ((h + 1) * (w + 1) * 16 - 16 * h * w)
    # the indexing of test_loss_backward_band_kernel_vs_tile_kernel_and_oracle: pixel (y, x) -> cell ((y + 2) // 4, (x + 2) // 4)
    v = torch.arange(8 * 12, dtype=F64).reshape(1, 8, 12)
    assert R.lse_layout(v, 2, 3)[0, 0 * 4 + 0, 2 * 4 + 2].item() == v[0, 0, 0].item()
    assert R.lse_layout(v, 2, 3)[0, 1 * 4 + 1, 0].item() == v[0, 2, 2].item()


def test_tables_are_well_formed():
    ids = [c['id'] for c in GPU_CASES]
    assert len(set(ids)) == len(ids) and 200 <= len(ids) <= 400, len(ids)
    assert {c['path'] for c in GPU_CASES} == set(R.PATH_ENV)
    assert {c['C'] for c in GPU_CASES if c['path'] == 'r4' and (c['h'], c['w']) == (9, 10)} >= set(R.R4_CLASS_COUNTS)
    assert {(c['h'], c['w']) for c in GPU_CASES if c['path'] == 'r4' and c['C'] == 150} >= set(R.R4_MAPS)
    for c in GPU_CASES + CPU_CASES:
        assert c['B'] <= 3 and c['h'] <= 24 and c['w'] <= 24 and c['H'] <= 96 and c['W'] <= 96, c['id']
        for dtype in R.dtypes_of(c):
            inp = R.inputs(c, dtype)
            assert torch.isfinite(inp['lo']).all(), c['id']
            t = inp['t']
            assert (((t >= 0) & (t < c['C'])) | (t == R.IGNORE)).all() and (t != R.IGNORE).any(), c['id']
            assert inp['cw'] is None or (torch.isfinite(inp['cw']).all() and (inp['cw'] >= 0).all()), c['id']
            if c['cw'] == 'zero2':
                present = torch.unique(t[t != R.IGNORE])
                assert int((inp['cw'][present] == 0).sum()) == min(2, len(present)), c['id']
            if c['lab'] == 'absent' and c['C'] > 1:
                assert not (t[0] == 1).any(), c['id']


def test_cached_K_is_what_the_statements_measure():
    """K of tests/loss_refs.py is the references' own error over the tables, re-derived here (torch's fp32 kernels differ a little
    between CPUs: the cached value must be within a quarter of what this machine measures, and never far above it)."""
    k32, kbf = R.measure_K(CPU_CASES + GPU_CASES)
    print('measured K', k32, kbf)
    for gm in k32:
        for name, v in k32[gm].items():
            if gm == 'generic' and name == 'lse':
                continue                                    # (no log-sum buffer outside ratio 4)
            assert v <= 1.25 * R.K32[gm][name] and R.K32[gm][name] <= 2.0 * v, (gm, name, v, R.K32[gm][name])
    for name, v in kbf.items():
        assert v <= 1.25 * R.KBF[name] and R.KBF[name] <= 2.0 * v, (name, v, R.KBF[name])


def _stmt_verdicts(c, dtype, ref, st, only):
    return R.judge(_entries(c, dtype, ref), st, c['id'], only=only)


@pytest.mark.parametrize('dtype', (F32, BF), ids=_name)
def test_unmutated_statements_are_accepted(dtype):
    """stmt32 on every CPU case in both storage types, stmt_bf16tile on the bf16 ratio-4 ones, inside the bound of their path."""
    for c in CPU_CASES:
        inp, ref = _ref(c, dtype)
        args = (inp['lo'], inp['t'], inp['cw'], c['go'], c['dice'])
        c32 = dict(c, path='r1' if c['path'] != 'generic' else 'generic')               # stmt32 takes exact maxima and fp32 sums
        v = R.judge(R.entries(ref, dtype, R.geom_class(c), bound='exact'), R.stmt32(*args), c32['id'])
        assert all(v.values()), [x.message for x in v.values() if not x.ok]
        if _is_tile(c, dtype):
            v = R.judge(R.entries(ref, dtype, 'pow2', tile_fwd=True, tile_bwd=True), R.stmt_bf16tile(*args), c['id'], only=('grad', 'P', 'loss'))
            assert all(v.values()), [x.message for x in v.values() if not x.ok]


@pytest.mark.parametrize('mut', R.MUTANTS)
def test_mutant_is_rejected(mut):
    """Each wrong computation is outside the bound, in fp32 AND under the looser bf16-tile bound, on at least one CPU case where the
    unmutated reference statements are inside it."""
    for dtype in (F32, BF):
        killed = []
        for c in CPU_CASES:
            if dtype == BF and not c['path'].startswith('r4'):
                continue
            inp, ref = _ref(c, dtype)
            args = (inp['lo'], inp['t'], inp['cw'], c['go'], c['dice'])
            en = R.entries(ref, dtype, R.geom_class(c), tile_fwd=dtype == BF, tile_bwd=dtype == BF)
            bad = R.statement(*args, mut=mut)
            if all(R.judge(en, bad, c['id']).values()):
                continue
            ok = all(R.judge(R.entries(ref, dtype, R.geom_class(c), bound='exact'), R.stmt32(*args), c['id']).values())
            if dtype == BF:
                ok = ok and all(R.judge(en, R.stmt_bf16tile(*args), c['id'], only=('grad', 'P', 'loss')).values())
            if ok:
                killed.append(c['id'])
                break
        assert killed, (mut, _name(dtype))


def test_sets0_rule_is_not_observable():
    """`sets == 0 -> denominator 2 I` changes no output (tests/loss_refs.py, EQUIVALENT_MUTANTS): bitwise, on the cases that have an image
    without valid pixels and on the all-ignored batch."""
    cases = [c for c in CPU_CASES if c['lab'] == 'image_ignored'] + [R.case('r4', 2, 19, 5, 6, 20, 24, lab='all_ignored')]
    assert len(cases) >= 3
    for c in cases:
        inp, ref = _ref(c, F32)
        mutd = R.statement(inp['lo'], inp['t'], inp['cw'], c['go'], c['dice'], mut='no_sets0_rule')
        assert (ref['P'] + ref['T'] == 0).any(), c['id']
        for name in ('loss', 'grad', 'I', 'P', 'T'):
            assert torch.equal(torch.nan_to_num(ref[name], nan=-1.0), torch.nan_to_num(mutd[name], nan=-1.0)), (c['id'], name)


# ---- CPU: the path table ---------------------------------------------------------------------------------------------------------------
def _dry(c, dtype, monkeypatch):
    """Dry runs of segf_ce_dice_fwd / segf_ce_dice_bwd with the arguments hip.ce_dice_fwd / hip.ce_dice_bwd would pass."""
    from segmentation_factory_amd import dispatch, hip
    for k, v in c['env'].items():
        monkeypatch.setenv(k, v)
    try:
        dt = hip.F32 if dtype == F32 else hip.BF16
        ld, front = R.ld_of(c)
        ptr = 'p%d' % (front * (4 if dtype == F32 else 2))
        geo = [dt, c['B'], c['C'], c['h'], c['w'], c['H'], c['W']]
        nl = hip.lib().segf_ce_dice_lse_floats(*geo, dispatch._PLACEHOLDER + int(ptr[1:]), ld) if _is_tile(c, dtype) else 0
        lse = 'p0' if nl else None
        rf, kf = dispatch.replay_rc({'fn': 'segf_ce_dice_fwd', 'args': geo + [ptr, ld, 'p0', R.IGNORE, None, 1, 'p0', 'p0', lse, None]})
        rb, kb = dispatch.replay_rc({'fn': 'segf_ce_dice_bwd', 'args': geo + [ptr, ld, 'p0', R.IGNORE, None, 1, 'p0', 'p0', 'p0', ld, 'p0', lse, None]})
    finally:
        for k in c['env']:
            monkeypatch.delenv(k)
    return rf, R.loss_kernels(kf), rb, R.loss_kernels(kb), nl


def test_every_row_reaches_the_kernels_it_is_meant_for(monkeypatch):
    """Dry runs (no device): the loss kernels a row launches are exactly the ones its path names, template arguments included."""
    seen = set()
    for c in GPU_CASES:
        for dtype in R.dtypes_of(c):
            rf, kf, rb, kb, nl = _dry(c, dtype, monkeypatch)
            wf, wb = R.expected_kernels(c, dtype)
            assert (rf, kf, rb, kb) == (0, wf, 0, wb), (c['id'], _name(dtype), kf, kb)
            assert bool(nl) == (R.band_covers(c, dtype) and c['path'] != 'r4_nolse'), c['id']
            seen.update(kf + kb)
    want = ['ce_dice_bwd_band_kernel<10, true, true>', 'ce_dice_bwd_band_kernel<2, false, false>', 'ce_dice_fwd_band_kernel<12, true>',
            'ce_dice_bwd_mfma4_kernel<T, 4> [T = float]', 'ce_dice_bwd_mfma4_kernel<T, 12> [T = unsigned short]',
            'ce_dice_fwd_cells16_kernel<T, 1, 4> [T = unsigned short]', 'ce_dice_bwd_cells8_kernel<T, 3, 8> [T = float]',
            'ce_dice_fwd_kernel<T, 2> [T = float]', 'bilinear_bwd_kernel<T>']
    assert not [k for k in want if k not in seen]
    for NT in (2, 4, 10, 12):
        for full in ('true', 'false') if NT < 12 else ('true',):          # (12 tiles: C > 160, the first 128 classes are always full)
            assert f'ce_dice_fwd_band_kernel<{NT}, {full}>' in seen and f'ce_dice_bwd_band_kernel<{NT}, {full}, true>' in seen
        assert f'ce_dice_fwd_mfma4_kernel<T, {NT}> [T = float]' in seen


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def _matrix_pipe(c):
    return c['path'] in ('r4', 'r4_nolse', 'r4_rows8', 'r4_tile')


def _derived(c, dtype, ref):
    """DERIVED terms of single paths (the module docstring lists them).
    generic, bf16: segf_ce_dice_bwd stages the full-resolution gradient in the storage type (include/segfac.h) before the transposed
        resize: every pixel's dz is rounded to bf16, |error| <= 2^-8 |dz| (half a unit in the last place of a bf16 value is at most
        2^-8 of it), and the resize adds them with its weights.
    ratio-4 matrix-pipe kernels (f32 MFMA, bf16 tile, band): the scale log2(e) rides in the interpolation's A operand (w * log2 e,
        rounded), so a logit in the exp2 domain carries a rounding relative to ITS OWN size, not to its distance from the maximum:
        log-sum - z_t moves by 2 * 2^-24 (|log-sum| + |z_t|) per pixel (the `offset` inputs: 200 * 2^-24 * 2, not 8 * 2^-24)."""
    d = {}
    if c['path'] == 'generic' and dtype == BF:
        d['grad'] = 2.0 ** -8 * ref['stage_abs']
    if _matrix_pipe(c):
        d['ce_sum'] = 2 * R.U24 * ref['D_ce_abs']
        per = d['ce_sum'].sum() / ref['w_sum'].sum()
        d['loss'] = torch.stack([per, per, torch.zeros_like(per)])
    return d


PAD_FILL = 3.0          # foreign columns in front of a view and pad columns behind the classes, where the row is wider than round8(C)


def _device_inputs(c, dtype, inp):
    B, C, h, w = c['B'], c['C'], c['h'], c['w']
    ld, front = R.ld_of(c)
    buf = torch.full((B * h * w, ld), PAD_FILL if c['ld'] in ('r8+8', 'view8', 'off4') else 0.0, dtype=dtype)
    buf[:, front:front + C] = inp['lo'].permute(0, 2, 3, 1).reshape(B * h * w, C).to(dtype)
    buf = buf.cuda()
    return buf, buf[:, front:front + C], inp['t'].cuda(), None if inp['cw'] is None else inp['cw'].float().cuda()


def _split(stats, B, C):
    s = stats[:B * (3 * C + 4)].view(B, 3 * C + 4).cpu()
    return dict(I=s[:, :C], P=s[:, C:2 * C], T=s[:, 2 * C:3 * C], ce_sum=s[:, 3 * C], w_sum=s[:, 3 * C + 1], n_valid=s[:, 3 * C + 2])


def _flags(stats):
    return [int(v) for v in stats[-4:].view(torch.int32).cpu()]


def _run(c, dtype, traced=False):
    """One forward + backward through hip.ce_dice_fwd / hip.ce_dice_bwd under the case's switches (the caller has set them)."""
    from segmentation_factory_amd import hip
    inp = R.inputs(c, dtype)
    buf, tok, tg, cw = _device_inputs(c, dtype, inp)
    keep = buf.clone()
    geo = (c['B'], c['C'], c['h'], c['w'], c['H'], c['W'])
    go = torch.full((1,), c['go'], device='cuda')
    with hip.trace() as tf:
        loss, stats, lse = hip.ce_dice_fwd(tok, *geo, tg, R.IGNORE, cw, c['dice'], want_lse=True)
    torch.cuda.synchronize()
    out = dict(loss=loss.cpu(), flags_fwd=_flags(stats), lse=None if lse is None else lse.cpu().clone(), **_split(stats, c['B'], c['C']))
    with hip.trace() as tb:
        d = hip.ce_dice_bwd(tok, *geo, tg, R.IGNORE, cw, c['dice'], stats, go, lse=lse)
    torch.cuda.synchronize()
    out.update(flags_bwd=_flags(stats), dlow=d.cpu(), grad=d[:, :c['C']].float().cpu(), kernels=(R.loss_kernels(tf.kernels), R.loss_kernels(tb.kernels)),
               untouched=torch.equal(buf, keep), inp=inp)
    return out


def _set_env(c, monkeypatch):
    for k, v in c['env'].items():
        monkeypatch.setenv(k, v)


GPU_PARAMS = [pytest.param(c, dt, id=f'{c["id"]}-{_name(dt)}') for c in GPU_CASES for dt in R.dtypes_of(c)]


@pytest.mark.gpu
@pytest.mark.parametrize('c,dtype', GPU_PARAMS)
def test_loss_kernels_against_float64(c, dtype, monkeypatch):
    _set_env(c, monkeypatch)
    a = _run(c, dtype)
    b = _run(c, dtype)
    B, C = c['B'], c['C']
    ref = R.statement(a['inp']['lo'], a['inp']['t'], a['inp']['cw'], c['go'], c['dice'])
    en = _entries(c, dtype, ref, _derived(c, dtype, ref))
    verdicts = R.judge(en, a, c['id'])
    if a['lse'] is not None and a['flags_fwd'][1] == 0:
        le = R.lse_entry(ref)
        verdicts['lse'] = R.compare(a['lse'].view(le['ref'].shape), le['ref'], le['e'], le['scale'], F32, 'elementwise', f'{c["id"]} lse',
                                    margin=R.MARGIN, floor=0.0, keep=le['keep'], extra=le['extra'])
    for name, v in verdicts.items():
        print(f'RATIO {c["path"]} {name} {c["id"]} {_name(dtype)} {v.ratio:.4g}')
    # the path, the exact outputs, reproducibility, the buffers around the operands
    assert a['kernels'] == tuple(R.expected_kernels(c, dtype)), a['kernels']
    assert torch.equal(a['T'].double(), ref['T']) and torch.equal(a['n_valid'].double(), ref['n_valid'])
    for name in ('loss', 'I', 'P', 'T', 'ce_sum', 'w_sum', 'n_valid', 'dlow'):
        assert torch.equal(torch.nan_to_num(a[name], nan=-7.0), torch.nan_to_num(b[name], nan=-7.0)), f'{name}: two runs differ'
    assert (a['lse'] is None) == (b['lse'] is None) and (a['lse'] is None or a['flags_fwd'][1] != 0 or torch.equal(a['lse'], b['lse']))
    assert a['untouched'], 'the logits buffer (the columns around the view included) was written'
    assert a['dlow'].shape == (B * c['h'] * c['w'], R.ld_of(c)[0]) and not a['dlow'][:, C:].any(), 'pad columns of the gradient'
    assert (a['lse'] is not None) == (R.band_covers(c, dtype) and c['path'] != 'r4_nolse')
    if c['inp'] == 'spike' and R.has_retry(c):              # (the per-pixel and generic paths have no flag: they never write the slot)
        assert a['flags_fwd'][0] == 0 and a['flags_bwd'][0] == 0
    if c['inp'] == 'spike_over' and R.has_retry(c):
        assert a['flags_fwd'][0] != 0 and a['flags_bwd'][0] != 0
        assert a['lse'] is None or a['flags_fwd'][1] != 0, 'the log-sum buffer of a flagged forward must be marked unusable'
    if not c['dice']:
        assert a['loss'][2].item() == 0.0 and a['loss'][0].item() == a['loss'][1].item()
    if c['lab'] == 'image_ignored':
        rows = c['h'] * c['w']
        assert not a['grad'][(B - 1) * rows:].any() and not a['P'][B - 1].any() and not a['I'][B - 1].any()
    if c['go'] == 0.0:
        assert not a['grad'].any()
    bad = [v.message for v in verdicts.values() if not v.ok]
    assert not bad, '\n'.join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', (F32, BF), ids=_name)
def test_uniform_class_weights_equal_none_bitwise(dtype, monkeypatch):
    for path, geo in (('r4', (2, 19, 9, 10, 36, 40)), ('r2', (2, 19, 5, 9, 10, 18)), ('generic', (2, 19, 5, 7, 18, 23))):
        base = R.case(path, *geo, go=1.7)
        ones = dict(base, cw='ones')                        # same id -> same seed -> same logits and labels
        a, b = _run(base, dtype), _run(ones, dtype)
        for name in ('loss', 'I', 'P', 'T', 'ce_sum', 'w_sum', 'n_valid', 'dlow'):
            assert torch.equal(a[name], b[name]), (path, name)


@pytest.mark.gpu
def test_bf16_paths_share_counts_and_segments_do_not_change_bits(monkeypatch):
    """The same bf16 input through every ratio-4 path: T, the counts and the weights are bitwise equal (as
    test_loss_backward_band_kernel_vs_tile_kernel_and_oracle asserts for two of them); three segments (h = 17, 8 rows each) give the
    bits of the default segment length."""
    base = R.case('r4', 2, 19, 17, 14, 68, 56, cwk='rand', go=1.7)
    outs = {}
    for path, env in R.PATH_ENV.items():
        if not path.startswith('r4'):
            continue
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        outs[path] = _run(dict(base, path=path, env=env), BF)
        assert outs[path]['kernels'] == tuple(R.expected_kernels(dict(base, path=path), BF)), path
        for k in env:
            monkeypatch.delenv(k)
    for path, o in outs.items():
        # w_sum is a float sum of random weights: the matrix-pipe kernels add it in one order (quad leaders, then the wave), the VALU
        # cells kernel in another, so there it is held to the bound (test_loss_kernels_against_float64) and to unit weights below
        for name in ('T', 'n_valid') + (('w_sum',) if _matrix_pipe(dict(path=path)) else ()):
            assert torch.equal(o[name], outs['r4'][name]), (path, name)
    unit = R.case('r4', 2, 19, 17, 14, 68, 56, go=1.7)
    first = None
    for path, env in R.PATH_ENV.items():
        if path.startswith('r4'):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            o = _run(dict(unit, path=path, env=env), BF)
            for k in env:
                monkeypatch.delenv(k)
            first = first or o
            for name in ('T', 'w_sum', 'n_valid'):
                assert torch.equal(o[name], first[name]), (path, name)
    for name in ('loss', 'I', 'P', 'ce_sum', 'dlow', 'lse'):
        assert torch.equal(outs['r4_rows8'][name], outs['r4'][name]), name


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', (F32, BF), ids=_name)
def test_all_ignored_batch_is_what_autograd_returns(dtype, monkeypatch):
    """No valid pixel in the whole batch: loss = {NaN, NaN, 0} (0 / 0 like F.cross_entropy; every Dice term is 1) and a gradient of exact
    zeros -- float64 autograd's answer (test_all_ignored_batch_statement_is_autograds) -- on every path."""
    rows = [('r1', (2, 19, 5, 6, 5, 6)), ('r2', (2, 19, 5, 6, 10, 12)), ('r8', (2, 19, 5, 6, 40, 48)), ('generic', (2, 19, 5, 6, 15, 18))]
    rows += [(p, (2, 19, 5, 6, 20, 24)) for p in R.PATH_ENV if p.startswith('r4') and (dtype == BF or p in ('r4', 'r4_nomfma'))]
    bad = []
    for path, geo in rows:
        c = R.case(path, *geo, lab='all_ignored', env=R.PATH_ENV[path])
        _set_env(c, monkeypatch)
        a = _run(c, dtype)
        for k in c['env']:
            monkeypatch.delenv(k)
        nan = int(torch.isnan(a['grad']).sum())
        print(f'ALLIGNORED {path} {_name(dtype)} loss {a["loss"].tolist()} grad NaNs {nan} nonzero {int((a["grad"] != 0).sum())}')
        if not (math.isnan(a['loss'][0].item()) and math.isnan(a['loss'][1].item()) and a['loss'][2].item() == 0.0 and not a['dlow'].any()):
            bad.append(path)
    assert not bad, bad
