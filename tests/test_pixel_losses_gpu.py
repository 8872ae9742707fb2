"""GPU checks of the per-pixel loss kernels (csrc/loss_pixel.hip) and of the loss classes built on them, against the float64
restatement of tests/pixel_loss_refs.py and the reference's recorded values (tests/golden/pixel_loss_cases.npz).

Inputs are rounded to the storage type first; the bars are those of tests/test_kernels_gpu.py::_close (fp32 2e-5 scale + 2e-7, bf16
3e-2 scale + 3e-4).  The CE map is held to the fp32 bar for BOTH storage types (the kernels interpolate and reduce in fp32 whatever the
storage).  The integers, kappa, the loss and the gradient are checked against the selection made on the kernel's OWN CE map, so no check
depends on which side of the decision value a borderline pixel falls."""
import functools
import math
import types

import numpy as np
import pytest
import torch

import pixel_loss_refs as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
DTYPES = [torch.float32, torch.bfloat16]
IDS = ['fp32', 'bf16']
SHAPES = [(2, 19, 8, 12, 32, 48),        # ratio 4; C not a multiple of 8
          (1, 150, 8, 8, 32, 32),        # three 64-class slices
          (1, 192, 4, 4, 16, 16),        # the class limit
          (2, 7, 16, 16, 32, 32),        # ratio 2
          (1, 3, 9, 11, 36, 44),         # tiles that overhang the map
          (2, 5, 24, 24, 24, 24),        # ratio 1
          (2, 5, 19, 25, 75, 100),       # non-dyadic: staged path
          (2, 19, 32, 32, 128, 128)]     # several workgroups in every selection pass
MODES = ['ohem', 'ohem_confident', 'ohem_weighted', 'focal_025_2', 'focal_1_0']
THETA = R.theta_of(0.7)


def _bar(dtype, scale):
    return (2e-5 * scale + 2e-7) if dtype == torch.float32 else (3e-2 * scale + 3e-4)


def _round(lo, dtype):
    return lo.to(dtype).float()


@functools.lru_cache(maxsize=None)
def _inputs(geom, mode, dtype):
    """(lo [B, h, w, C] fp32 holding storage-type values, labels, class weights): computed once, never modified."""
    seed = 7000 + 10 * SHAPES.index(geom) + MODES.index(mode) if geom in SHAPES else 6000
    if mode == 'ohem_confident':
        lo, t = R.confident_inputs(geom, seed, 9.0 if geom[1] >= 150 else 6.0)
    else:
        lo, t = R.plain_inputs(geom, seed)
    cw = R.random_weights(geom[1], seed + 1) if mode == 'ohem_weighted' else None
    return _round(lo, dtype), t, cw


@functools.lru_cache(maxsize=None)
def _ref_ce(geom, mode, dtype):
    lo, t, cw = _inputs(geom, mode, dtype)
    return R.ce(lo.to(F64), t, cw)[0]


def _run(lo, t, geom, mode, dtype, cw=None, go=None, ld=None):
    """One forward + backward through functional.upsample_pixel_loss: (loss, ce_map, info dict, d low [B, h, w, C]) on the host."""
    from segmentation_factory_amd import functional as Fh
    B, C, h, w, H, W = geom
    rows = lo.reshape(B * h * w, C).to(dtype)
    if ld is not None:                                   # a column slice of a wider buffer
        wide = torch.full((B * h * w, ld), 7.0, dtype=dtype)
        wide[:, :C] = rows
        x = wide.cuda()[:, :C].requires_grad_(True)
    else:
        x = rows.cuda().requires_grad_(True)
    kind, params = ('focal', (0.25, 2.0, True) if mode == 'focal_025_2' else (1.0, 0.0, True)) if mode.startswith('focal') else ('ohem', (THETA,))
    loss, ce_map, info = Fh.upsample_pixel_loss(x, t.cuda(), geom, kind, params, R.IGNORE, None if cw is None else cw.cuda())
    assert not ce_map.requires_grad and not info.requires_grad
    (loss if go is None else loss * go).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), ce_map.cpu(), Fh.pixel_loss_info(info), x.grad.float().cpu().view(B, h, w, C)


def _check(geom, mode, dtype, lo, t, cw, ref_ce, go=None, ld=None, want_topk=None):
    loss, ce_map, info, dlow = _run(lo, t, geom, mode, dtype, cw, go, ld)
    gof = 1.0 if go is None else go
    # 1. the CE map: fp32 bar for both storage types; every value a non-negative float with the sign bit clear
    e_ce, s_ce = float((ce_map.to(F64) - ref_ce).abs().max()), float(ref_ce.abs().max())
    print(f'  {geom} {mode} {dtype}: ce map err {e_ce:.3e} (scale {s_ce:.3e}, bar {_bar(torch.float32, s_ce):.3e})')
    assert e_ce <= _bar(torch.float32, s_ce)
    assert int((ce_map.view(torch.int32) < 0).sum()) == 0
    # 2. integers / kappa / loss from the kernel's own map
    if mode.startswith('focal'):
        f = R.focal(ce_map, *((0.25, 2.0) if mode == 'focal_025_2' else (1.0, 0.0)))
        want_loss, coef = f['loss'], f['coef']
        assert info['n_valid'] == int((t != R.IGNORE).sum()) and info['bad_label'] == 0
    else:
        sel = R.ohem(ce_map, t, THETA)
        want_loss, coef = sel['loss'], sel['coef']
        got = {k: info[k] for k in ('n_valid', 'n_min', 'n_hard', 'n_gt', 'n_eq', 'used_topk')}
        print(f'    info {info}')
        assert got == {k: sel[k] for k in got}, (got, sel)
        if sel['used_topk']:
            kap = torch.topk(ce_map.flatten(), sel['n_min']).values[-1]
            assert np.float32(info['kappa']).tobytes() == kap.numpy().tobytes()
        else:
            assert np.float32(info['kappa']) == np.float32(THETA)
        if want_topk is not None:
            assert sel['used_topk'] == want_topk
    if math.isnan(float(want_loss)):
        assert math.isnan(float(loss))
    else:
        e_l = abs(float(loss) - float(want_loss)) / abs(float(want_loss))
        print(f'    loss {float(loss):.7f} want {float(want_loss):.7f} rel err {e_l:.2e}')
        assert e_l <= 2e-5
    # 3. the gradient of the low-resolution logits, with the coefficients derived from the kernel's map
    want = R.grad_low(lo.to(F64), t, coef, cw, gof)
    e_g, s_g = float((dlow.to(F64) - want).abs().max()), float(want.abs().max())
    print(f'    d low err {e_g:.3e} (scale {s_g:.3e}, bar {_bar(dtype, s_g):.3e})')
    assert e_g <= _bar(dtype, s_g)
    return loss, ce_map, info, dlow


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('geom', SHAPES, ids=lambda g: 'x'.join(map(str, g)))
def test_pixel_loss_against_float64(geom, mode, dtype):
    lo, t, cw = _inputs(geom, mode, dtype)
    want_topk = {'ohem': 0, 'ohem_weighted': 0, 'ohem_confident': 1}.get(mode)
    _check(geom, mode, dtype, lo, t, cw, _ref_ce(geom, mode, dtype), want_topk=want_topk)


# ---- the reference's recorded values ------------------------------------------------------------------------------------------------
def _class_of(name, case):
    from segmentation_factory_amd import losses
    cw = case['weight'].tolist() if 'weight' in case else None
    if name.startswith('ohem'):
        return losses.OhemCrossEntropy(R.IGNORE, cw, thresh=float(case['params'][0]), aux_weights=case['aux'].tolist())
    if name.startswith('focal'):
        return losses.FocalLoss(float(case['params'][0]), float(case['params'][1]))
    return losses.CrossEntropy(R.IGNORE, cw)


@pytest.mark.parametrize('path', ['lowres', 'nchw'])
def test_fixture_cases_against_the_reference(path):
    """Every fixture case through the low-resolution path and through the NCHW path (full-resolution logits made by the library's own
    resize), fp32, against the reference's recorded loss within 1e-4 relative: in the threshold branch the tool asserted that no pixel
    lies within 1e-3 of theta (the fp32 CE error is ~1e-6), in the top-k branch a swap of near-equal neighbours of kappa moves the mean
    by less than the CE-map error / n_min.  The low-resolution gradient is compared with the recorded autograd gradient as well."""
    from segmentation_factory_amd import functional as Fh
    from segmentation_factory_amd.backbones import TokenMap
    cases = R.load_golden()
    assert len(cases) == 14
    for name, case in sorted(cases.items()):
        B, C, h, w, H, W = (int(v) for v in case['geom'])
        t = torch.from_numpy(case['labels'].astype(np.int64)).cuda()
        lows = [torch.from_numpy(case[f'low{i}']).reshape(B * h * w, C).cuda().requires_grad_(True) for i in range(len(case['aux']))]
        if path == 'lowres':
            preds = tuple(TokenMap(x, B, h, w) for x in lows)
        else:
            preds = tuple(Fh.upsample_to_nchw(x, (B, C, h, w, H, W)) for x in lows)
        loss = _class_of(name, case)(preds if len(preds) > 1 else preds[0], t)
        loss.backward()
        e_l = abs(loss.item() - float(case['loss'])) / abs(float(case['loss']))
        e_g = max(float((x.grad.cpu().view(B, h, w, C) - torch.from_numpy(case[f'dlow{i}'])).abs().max()) /
                  float(np.abs(case[f'dlow{i}']).max()) for i, x in enumerate(lows))
        print(f'  {name} [{path}]: loss {loss.item():.7f} reference {float(case["loss"]):.7f} rel err {e_l:.2e}; d low err/scale {e_g:.2e}')
        assert e_l <= 1e-4, name
        if int(case.get('branch', 0)) == 0:           # top-k ties / near-ties: the reference's choice among them is not pinned
            assert e_g <= 1e-4, name


# ---- trace and reproducibility ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_trace_names_the_kernels_and_runs_are_bit_identical(dtype):
    from segmentation_factory_amd import hip
    for geom, mode, fwd, bwd in (((2, 19, 8, 12, 32, 48), 'ohem_confident', 'pixel_loss_fwd_cells_kernel', 'pixel_loss_bwd_cells_kernel'),
                                 ((2, 5, 19, 25, 75, 100), 'ohem', 'pixel_loss_fwd_kernel', 'pixel_loss_bwd_kernel'),
                                 ((2, 7, 16, 16, 32, 32), 'focal_025_2', 'pixel_loss_fwd_cells_kernel', 'pixel_loss_bwd_cells_kernel')):
        lo, t, cw = _inputs(geom, mode, dtype)
        B, C, h, w, H, W = geom
        x, tt = lo.reshape(B * h * w, C).to(dtype).cuda(), t.cuda()
        code, p0, p1 = (hip.PIXEL_FOCAL, 0.25, 2.0) if mode.startswith('focal') else (hip.PIXEL_OHEM, THETA, 0.0)
        with hip.trace() as tr:         # (the trace is per thread: autograd would run the backward on another one)
            _, ce_map, state = hip.pixel_loss_fwd(x, B, C, h, w, H, W, tt, R.IGNORE, None, code, p0, p1, 1)
            hip.pixel_loss_bwd(x, B, C, h, w, H, W, tt, R.IGNORE, None, code, p0, p1, 1, ce_map, state, torch.ones(1, device='cuda'))
        names = [k.split('<')[0] for k in tr.kernels]
        assert fwd in names and bwd in names and 'pixel_loss_finalize_kernel' in names, names
        if mode.startswith('ohem'):
            assert names.count('pixel_loss_select_hist_kernel') == 4 and 'pixel_loss_topk_final_kernel' in names
        a = _run(lo, t, geom, mode, dtype, cw)
        b = _run(lo, t, geom, mode, dtype, cw)
        assert a[0].numpy().tobytes() == b[0].numpy().tobytes()
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and a[2] == b[2]
        assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))


# ---- edge cases -------------------------------------------------------------------------------------------------------------------
def _edge(kind, dtype):
    g = torch.Generator().manual_seed(11)
    if kind in ('all_ignored', 'valid15_none_hard', 'valid15_three_hard'):
        geom = (1, 5, 4, 4, 16, 16)
        lo = torch.randn(1, 4, 4, 5, generator=g)
        t = torch.full((1, 16, 16), R.IGNORE, dtype=torch.int64)
        if kind != 'all_ignored':
            lo[..., 2] += 12.0
            pos = torch.randperm(256, generator=g)[:15]
            t.view(-1)[pos] = 2
            if kind == 'valid15_three_hard':
                t.view(-1)[pos[:3]] = 0
    elif kind in ('n_hard_eq_n_min', 'n_hard_eq_n_min_minus_1'):
        geom = (1, 5, 8, 8, 8, 8)
        lo = torch.randn(1, 8, 8, 5, generator=g)
        t = torch.randint(0, 5, (1, 8, 8), generator=g)
        lo.scatter_add_(-1, t[..., None], torch.full((1, 8, 8, 1), 9.0))
        for p in torch.randperm(64, generator=g)[:4 if kind == 'n_hard_eq_n_min' else 3].tolist():
            lo.view(64, 5)[p, int(t.view(-1)[p])] -= 12.0
    elif kind == 'constant_topk':
        geom = (1, 5, 4, 4, 16, 16)
        lo = torch.zeros(1, 4, 4, 5)
        lo[..., 1] = 3.0                                  # ce = log(4 + e^3) - 3 = 0.18 < theta everywhere: top-k over equal values
        t = torch.ones(1, 16, 16, dtype=torch.int64)
    else:
        raise KeyError(kind)
    return geom, _round(lo, dtype), t


EDGES = ('all_ignored', 'valid15_none_hard', 'valid15_three_hard', 'n_hard_eq_n_min', 'n_hard_eq_n_min_minus_1', 'constant_topk')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind', EDGES)
def test_ohem_edge_cases(kind, dtype):
    geom, lo, t = _edge(kind, dtype)
    ref_ce = R.ce(lo.to(F64), t)[0]
    loss, ce_map, info, dlow = _check(geom, 'ohem', dtype, lo, t, None, ref_ce)
    if kind in ('all_ignored', 'valid15_none_hard'):
        assert math.isnan(float(loss)) and int((dlow != 0).sum()) == 0
        assert info['n_valid'] == (0 if kind == 'all_ignored' else 15) and info['n_hard'] == 0 and info['n_min'] == 0
    elif kind == 'valid15_three_hard':
        assert (info['n_valid'], info['n_min'], info['n_hard'], info['used_topk']) == (15, 0, 3, 0)
        hard = ce_map.flatten()[ce_map.flatten() > THETA]
        assert hard.numel() == 3 and abs(float(loss) - float(hard.double().mean())) <= 2e-5 * float(hard.double().mean())
    elif kind == 'n_hard_eq_n_min':
        assert (info['n_min'], info['n_hard'], info['used_topk']) == (4, 4, 0)
    elif kind == 'n_hard_eq_n_min_minus_1':
        assert (info['n_min'], info['n_hard'], info['used_topk'], info['n_gt'], info['n_eq']) == (4, 3, 1, 3, 1)
    else:
        assert (info['used_topk'], info['n_gt'], info['n_eq'], info['n_min']) == (1, 0, 256, 16)
        assert np.float32(float(loss)) == np.float32(info['kappa'])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('mode', ['ohem', 'ohem_confident', 'focal_025_2'])
def test_leading_dimension_and_grad_out(mode, dtype):
    """A column-slice view of a wider logits buffer (row stride 8 for 5 classes) and grad_out != 1."""
    geom = (1, 5, 4, 4, 16, 16)
    lo, t, cw = _inputs(geom, mode, dtype)
    ref_ce = R.ce(lo.to(F64), t)[0]
    a = _check(geom, mode, dtype, lo, t, None, ref_ce, go=-2.5, ld=8)
    b = _check(geom, mode, dtype, lo, t, None, ref_ce, go=-2.5)
    assert torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_backward_zeroes_the_pad_columns(dtype):
    from segmentation_factory_amd import hip
    for geom in ((1, 5, 4, 4, 16, 16), (1, 5, 5, 3, 16, 16)):                 # fused and staged backward
        B, C, h, w, H, W = geom
        lo, t, _ = _inputs(geom, 'ohem', dtype)
        wide = torch.full((B * h * w, 8), 7.0, dtype=dtype)
        wide[:, :C] = lo.reshape(-1, C).to(dtype)
        x = wide.cuda()[:, :C]
        tt = t.cuda()
        loss, ce_map, state = hip.pixel_loss_fwd(x, B, C, h, w, H, W, tt, R.IGNORE, None, hip.PIXEL_OHEM, THETA, 0.0, 1)
        go = torch.ones(1, device='cuda')
        d = hip.pixel_loss_bwd(x, B, C, h, w, H, W, tt, R.IGNORE, None, hip.PIXEL_OHEM, THETA, 0.0, 1, ce_map, state, go)
        assert d.shape == (B * h * w, 8) and int((d[:, C:] != 0).sum()) == 0 and float(d[:, :C].float().abs().max()) > 0


def test_out_of_range_labels_are_skipped_and_flagged():
    """As segf_ce_dice_fwd: skipped (no loss, no gradient, not counted valid) and flagged; nothing raised on the Python side."""
    geom = (1, 5, 4, 4, 16, 16)
    lo, t, _ = _inputs(geom, 'ohem', torch.float32)
    t = t.clone()
    t[0, 5, 5], t[0, 9, 3] = 5, -1
    loss, ce_map, info, dlow = _run(lo, t, geom, 'ohem', torch.float32)
    assert info['bad_label'] == 1 and float(ce_map[0, 5, 5]) == 0.0 and float(ce_map[0, 9, 3]) == 0.0
    t2 = t.clone()
    t2[0, 5, 5] = t2[0, 9, 3] = R.IGNORE
    loss2, ce2, info2, dlow2 = _run(lo, t2, geom, 'ohem', torch.float32)
    assert info2['bad_label'] == 0 and torch.equal(ce_map, ce2) and torch.equal(dlow, dlow2) and float(loss) == float(loss2)
    assert info['n_valid'] == info2['n_valid']


# ---- graph replay -----------------------------------------------------------------------------------------------------------------
def test_ohem_replays_either_branch_in_a_captured_graph():
    """Forward + backward of OhemCrossEntropy captured once on static buffers (one stream); replays with threshold-branch inputs, then
    top-k inputs, then threshold again are bit-equal to the eager results: the branch is taken on the device."""
    from segmentation_factory_amd import functional as Fh, losses
    from segmentation_factory_amd.backbones import TokenMap
    geom = (2, 19, 8, 12, 32, 48)
    B, C, h, w, H, W = geom
    sets = [_inputs(geom, m, torch.float32) for m in ('ohem', 'ohem_confident')]
    fn = losses.OhemCrossEntropy()

    def eager(lo, t):
        x = lo.reshape(B * h * w, C).cuda().requires_grad_(True)
        loss = fn(TokenMap(x, B, h, w), t.cuda())
        g, = torch.autograd.grad(loss, x)
        return loss.detach().clone(), g.clone(), Fh.pixel_loss_info(fn.last_info)
    want = [eager(lo, t) for lo, t, _ in sets]
    assert [w_[2]['used_topk'] for w_ in want] == [0, 1]

    sx = torch.zeros(B * h * w, C, device='cuda').requires_grad_(True)
    st = torch.zeros(B, H, W, dtype=torch.int64, device='cuda')
    sx.data.copy_(sets[0][0].reshape(-1, C)); st.copy_(sets[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(fn(TokenMap(sx, B, h, w), st), sx)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_loss = fn(TokenMap(sx, B, h, w), st)
        s_grad, = torch.autograd.grad(s_loss, sx)
    s_info = fn.last_info
    for which in (0, 1, 0):
        sx.data.copy_(sets[which][0].reshape(-1, C)); st.copy_(sets[which][1])
        graph.replay()
        torch.cuda.synchronize()
        info = Fh.pixel_loss_info(s_info)
        print(f'  replay with set {which}: loss {s_loss.item():.7f} used_topk {info["used_topk"]} n_hard {info["n_hard"]} n_min {info["n_min"]}')
        assert info == want[which][2]
        assert s_loss.detach().cpu().numpy().tobytes() == want[which][0].cpu().numpy().tobytes()
        assert torch.equal(s_grad.view(torch.int32), want[which][1].view(torch.int32))


# ---- model level ------------------------------------------------------------------------------------------------------------------
def _mit_b0(nc, seed=1234):
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel
    m = SegmentationModel('MiT-B0', num_classes=nc, seg_head='SegFormerHead', compute_dtype=torch.float32)
    m.load_state_dict(OW.make_state_dict('MiT-B0', 'SegFormerHead', nc, seed))
    m = m.cuda().train()
    for mod in m.modules():
        if hasattr(mod, 'drop_prob'):
            mod.drop_prob = 0.0
        if isinstance(mod, (torch.nn.Dropout, torch.nn.Dropout2d)):
            mod.p = 0.0
    return m


def test_model_lowres_and_nchw_paths_agree():
    from oracle import weights as OW
    from segmentation_factory_amd import OhemCrossEntropy
    nc, B, H, W = 7, 2, 64, 64
    x, y = OW.learnable_batch(B, H, W, nc, 9)
    m = _mit_b0(nc)
    fn = OhemCrossEntropy()
    a = fn(m.forward_lowres(x.cuda()), y.cuda()).item()
    b = fn(m(x.cuda()), y.cuda()).item()
    print(f'  OhemCrossEntropy: low-res path {a:.7f}, NCHW path {b:.7f}')
    assert math.isfinite(a) and abs(a - b) <= 1e-4 * abs(a)


@pytest.mark.parametrize('loss_name', ['OhemCrossEntropy', 'FocalLoss'])
def test_train_one_epoch_with_a_named_loss(loss_name, capsys):
    """Three steps of engine.train_one_epoch (MiT-B0 + SegFormerHead, 7 classes, 64 x 64, batch 2, fp32, stochastic rates 0) with
    args.loss set and hip_graph=True: one captured graph, finite losses, the first loss is the eager loss, every parameter moves."""
    from oracle import weights as OW
    from segmentation_factory_amd import engine, losses
    from segmentation_factory_amd.optim import FusedAGCAdamW, NativeScaler
    nc, B, H, W = 7, 2, 64, 64
    x, y = OW.learnable_batch(B, H, W, nc, 9)
    args = types.SimpleNamespace(nb_classes=nc, dice=True, ignore_index=255, ignore_label=255, local_rank=0, device='cuda', hip_graph=True,
                                 loss=loss_name, focal_gamma=2.0)
    fn = losses.OhemCrossEntropy() if loss_name == 'OhemCrossEntropy' else losses.FocalLoss(1.0, 2.0)
    l_eager = fn(_mit_b0(nc).forward_lowres(x.cuda()), y.cuda()).item()
    model = _mit_b0(nc)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    opt = FusedAGCAdamW(model.parameters(), lr=1e-3, weight_decay=0.0)
    seen = []

    class Rec:
        def add_scalar(self, name, v, it=None):
            if name == 'train_loss':
                seen.append(float(v))
    engine.train_one_epoch(model, opt, [(x, y)] * 3, 0, 'cuda', 1, None, None, NativeScaler(), Rec(), args)
    out = capsys.readouterr().out
    assert getattr(model, '_graphed_step', None) is not None and out.count('captured as one hipGraph') == 1
    print(f'  {loss_name}: graphed losses {seen}, eager first loss {l_eager:.7f}')
    assert len(seen) == 3 and all(np.isfinite(seen))
    assert abs(seen[0] - l_eager) <= 1e-5 * max(1.0, abs(l_eager))
    moved = [k for k, v in model.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert len(moved) == len(before), sorted(set(before) - set(moved))[:8]
