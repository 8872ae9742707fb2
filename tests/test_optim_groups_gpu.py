"""Per-group learning rate and weight decay in the fused optimizer steps (segf_agc_adamw_groups / segf_flat_optim_step_groups through
FusedAGCAdamW / FusedSGD / FusedAdam / FusedRMSprop) against torch.optim itself on the CPU with the same groups, step for step: four
groups with their own lr and weight decay (one with lr 0 and decay on, which must still update its state), every group's lr changed
between the steps by unequal factors, one parameter that never gets a gradient and one that misses a step; then a checkpoint handed
between the fused and the torch class in both directions, the uniform case on the scalar kernels, the step beside a replayed hipGraph
and the refusals of the raw entry points.

Bars: those of tests/test_optimizers_gpu.py for the same comparison -- max abs error < 2e-6 per step against torch for the parameters,
and for the state buffers relative to their largest entry; 1e-5 where AGC (restated in oracle/optim.py) is in front."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (5,), (4, 3, 2, 2), (9,), (3, 130)]       # (3, 130): rows of two lane strides plus a ragged tail of 2
GROUP_OF = [0, 1, 1, 3, 2]                                  # parameter -> group; parameter 2 never gets a gradient
WDS = [0.0, 0.05, 0.01, 0.3]
# every group's lr, per step: unequal factors from step to step, so no constant ratio between the groups can pass; group 3 sits at
# lr 0 with decay on for two steps (its state must move all the same) and is then switched on
LRS = [[1e-2, 3e-3, 1e-3, 0.0], [5e-3, 2.7e-3, 1.3e-3, 0.0], [4e-3, 9e-4, 1.6e-3, 2e-3], [1e-3, 1.2e-3, 8e-4, 5e-3]]
HAVE = [(0, 1, 3, 4), (0, 1, 3, 4), (0, 3, 4), (0, 1, 3, 4)]          # parameter 1 misses step 2
RULES = ['sgd', 'momentum', 'sgd_mu0', 'adam', 'rmsprop', 'rmsprop_mu0', 'agc_adamw']       # RULE_NAMES of test_optimizers_gpu + AdamW


def _pair(rule):
    """(fused class, torch class) constructors over a list of groups; the groups bring their own lr / weight_decay."""
    from segmentation_factory_amd.optim import FusedAdam, FusedAGCAdamW, FusedRMSprop, FusedSGD
    o = torch.optim
    return {
        'sgd': (lambda g: FusedSGD(g, momentum=0.9, nesterov=True), lambda g: o.SGD(g, lr=1e-3, momentum=0.9, nesterov=True)),
        'momentum': (lambda g: FusedSGD(g, momentum=0.9), lambda g: o.SGD(g, lr=1e-3, momentum=0.9)),
        'sgd_mu0': (lambda g: FusedSGD(g), lambda g: o.SGD(g, lr=1e-3)),
        'adam': (lambda g: FusedAdam(g), lambda g: o.Adam(g)),
        'rmsprop': (lambda g: FusedRMSprop(g, alpha=0.9, momentum=0.9), lambda g: o.RMSprop(g, alpha=0.9, momentum=0.9)),
        'rmsprop_mu0': (lambda g: FusedRMSprop(g, alpha=0.9), lambda g: o.RMSprop(g, alpha=0.9)),
        'agc_adamw': (lambda g: FusedAGCAdamW(g), lambda g: o.AdamW(g)),
    }[rule]


def _four_groups(ps, lrs=LRS[0], wds=WDS):
    return [{'params': [p for p, g in zip(ps, GROUP_OF) if g == k], 'lr': lrs[k], 'weight_decay': wds[k]} for k in range(4)]


def _setup(rule, seed=3, lrs=LRS[0], wds=WDS):
    make, make_ref = _pair(rule)
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in SHAPES]
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    return g, ps, ref, make(_four_groups(ps, lrs, wds)), make_ref(_four_groups(ref, lrs, wds))


def _assert_state_close(opt, ropt, bar):
    state, rstate = opt.state_dict()['state'], ropt.state_dict()['state']
    assert set(state) == set(k for k, v in rstate.items() if v)
    for k, st in state.items():
        assert set(st) == set(rstate[k])
        for name, v in st.items():
            want = torch.as_tensor(rstate[k][name]).float()
            err = (torch.as_tensor(v).float() - want).abs().max().item()
            assert err <= bar * max(1.0, want.abs().max().item()), (k, name, err)
    return state


@pytest.mark.parametrize('rule', RULES)
def test_group_step_matches_its_torch_class(rule):
    from segmentation_factory_amd import hip
    g, ps, ref, opt, ropt = _setup(rule)
    opt.set_clipping(None, 'agc')
    before = [p.detach().clone() for p in ps]
    for step, have in enumerate(HAVE):
        for o in (opt, ropt):
            for pg, lr in zip(o.param_groups, LRS[step]):
                pg['lr'] = lr
        for i, (p, r) in enumerate(zip(ps, ref)):
            gr = torch.randn(*SHAPES[i], generator=g) if i in have else None
            p.grad, r.grad = (None, None) if gr is None else (gr.cuda(), gr.clone())
        with hip.trace() as t:
            opt.step()
        assert len(t.kernels) == 1 and 'groups_kernel' in t.kernels[0], t.kernels        # one launch, of the group form
        ropt.step()
        errs = [(p.detach().cpu() - r.detach()).abs().max().item() for p, r in zip(ps, ref)]
        print(f'{rule} step {step}: max abs error per parameter {["%.2e" % e for e in errs]}')
        for i, e in enumerate(errs):
            assert e < 2e-6, (step, i, e)
        if step == 1:       # lr 0 with decay on: the parameter stands still ...
            assert torch.equal(ps[3].detach(), before[3])
    assert torch.equal(ps[2].detach(), before[2])                     # never a gradient: untouched, bit for bit
    assert not torch.equal(ps[3].detach(), before[3])                 # ... and moves once its group's lr is switched on
    state = _assert_state_close(opt, ropt, 2e-6)                      # ... on the state it gathered meanwhile, as torch's did
    packed = {0: 0, 1: 1, 3: 4, 4: 3}                                 # parameter -> packed index (group order); none for parameter 2
    assert 2 not in state and len(state) == (0 if rule == 'sgd_mu0' else 4)
    if rule in ('adam', 'rmsprop', 'agc_adamw'):
        assert float(state[packed[1]]['step']) == 3.0 and float(state[packed[0]]['step']) == 4.0 and float(state[packed[3]]['step']) == 4.0


@pytest.mark.parametrize('rule', ['sgd', 'rmsprop', 'agc_adamw'])
def test_agc_in_front_of_the_group_step(rule):
    """clip_mode 'agc' (0.02) inside the group kernels: oracle.optim.adaptive_clip_grad_ on the raw gradient (unit-wise, so the same
    for every group), then the torch class's step with the four groups."""
    from oracle import optim as OO
    g, ps, ref, opt, ropt = _setup(rule, seed=5)
    opt.set_clipping(0.02, 'agc')
    clipped = 0
    for step in range(3):
        for o in (opt, ropt):
            for pg, lr in zip(o.param_groups, LRS[step + 1]):
                pg['lr'] = lr
        for i, (p, r) in enumerate(zip(ps, ref)):
            gr = torch.randn(*SHAPES[i], generator=g) * 2
            p.grad = gr.cuda()
            r.grad = OO.adaptive_clip_grad_(r.detach(), gr.clone(), 0.02)
            clipped += int(not torch.equal(r.grad, gr))
        opt.step()
        ropt.step()
        for i, (p, r) in enumerate(zip(ps, ref)):
            err = (p.detach().cpu() - r.detach()).abs().max().item()
            print(f'{rule} agc step {step} parameter {i}: max abs error {err:.2e}')
            assert err < 1e-5, (step, i)
    assert clipped == 15                                               # every gradient was actually clipped
    _assert_state_close(opt, ropt, 1e-5)


def test_many_units_walk_the_grid_stride():
    """More units than the launch has waves (4096 workgroups x 4): 20000 rows in one group, 20000 in another and a 1-D tensor."""
    from segmentation_factory_amd.optim import FusedSGD
    g = torch.Generator().manual_seed(11)
    shapes = [(20000, 3), (20000, 2), (7,)]
    ref = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    ps = [torch.nn.Parameter(r.detach().clone().cuda()) for r in ref]
    groups = lambda l: [{'params': [l[0]], 'lr': 1e-2, 'weight_decay': 0.1}, {'params': [l[1]], 'lr': 3e-3, 'weight_decay': 0.02},
                        {'params': [l[2]], 'lr': 1e-3, 'weight_decay': 0.0}]
    opt, ropt = FusedSGD(groups(ps), momentum=0.9), torch.optim.SGD(groups(ref), lr=1.0, momentum=0.9)
    for _ in range(2):
        for p, r in zip(ps, ref):
            r.grad = torch.randn(r.shape, generator=g)
            p.grad = r.grad.cuda()
        opt.step()
        ropt.step()
    for p, r in zip(ps, ref):
        assert (p.detach().cpu() - r.detach()).abs().max().item() < 2e-6


@pytest.mark.parametrize('rule', RULES)
def test_checkpoint_round_trip_with_four_groups(rule):
    """Two steps of one class, its state_dict (four groups with their own lr / weight_decay, rewritten between the steps) loaded into
    the other class built with different hyper-parameters, one more step of both: fused -> torch and torch -> fused."""
    for fused_first in (True, False):
        g, ps, ref, opt, ropt = _setup(rule, seed=21)
        make, make_ref = _pair(rule)
        mine, theirs = (ps, ref) if fused_first else (ref, ps)
        first = opt if fused_first else ropt
        for step in range(2):
            for pg, lr in zip(first.param_groups, LRS[step + 1]):
                pg['lr'] = lr
            for p in mine:
                p.grad = torch.randn(p.shape, generator=g).to(p.device)
            first.step()
        for p, q in zip(mine, theirs):
            q.data.copy_(p.detach())
        wrong = _four_groups(theirs, lrs=[1.0] * 4, wds=[0.5] * 4)
        second = (make_ref if fused_first else make)(wrong)
        second.load_state_dict(first.state_dict())
        assert [(pg['lr'], pg['weight_decay']) for pg in second.param_groups] == list(zip(LRS[2], WDS))
        for p, q in zip(mine, theirs):
            gr = torch.randn(p.shape, generator=g)
            p.grad, q.grad = gr.to(p.device), gr.to(q.device)
        first.step()
        second.step()
        for p, q in zip(mine, theirs):
            assert torch.allclose(q.detach().cpu(), p.detach().cpu(), rtol=2e-6, atol=1e-7), (rule, fused_first)


@pytest.mark.parametrize('agc', [None, 0.02])
def test_uniform_groups_stay_on_the_scalar_kernels(agc):
    """Shared lr, decays {0, wd}: hip.trace() names only the kernels of segf_agc_adamw / segf_flat_optim_step, whatever lr_scale says;
    forcing the group entry point with the same per-group values gives the same bits in parameters and state -- both instantiations
    share their arithmetic."""
    from segmentation_factory_amd import hip
    for rule in RULES:
        runs = []
        for force in (False, True):
            g, ps, _, opt, _ = _setup(rule, seed=7, lrs=[2e-3] * 4, wds=[0.0, 0.05, 0.05, 0.0])
            opt.param_groups[2]['lr_scale'] = 1.0
            opt.force_groups = force
            opt.set_clipping(agc, 'agc')
            names = []
            for have in HAVE[1:]:
                for i, p in enumerate(ps):
                    p.grad = torch.randn(*SHAPES[i], generator=g).cuda() if i in have else None
                with hip.trace() as t:
                    opt.step()
                names += t.kernels
            assert len(names) == 3 and all(('groups_kernel' in n) == force for n in names), (rule, names)
            assert all(n.startswith(('agc_adamw_kernel', 'flat_optim_kernel<', '(flat_optim_kernel<')) for n in names) or force, names
            runs.append([p.detach().clone() for p in ps] + [getattr(opt, a).clone() for _, a in opt._state_spec(opt.param_groups[0])]
                        + [opt._ustep.clone()])
        for a, b in zip(*runs):
            assert torch.equal(a, b), rule


def test_graphed_group_step_matches_eager_step():
    """--head-lr-mult 10 through create_optimizer (FusedSGD, Nesterov) on the small model of
    test_optimizers_gpu.py::test_graphed_sgd_step_matches_eager_step: GraphedTrainStep -- the group step beside the replayed graph --
    walks the eager loss curve."""
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, criterion_lowres, hip
    from segmentation_factory_amd.graph import GraphedTrainStep
    from segmentation_factory_amd.optim import NativeScaler, create_optimizer
    backbone, head, nc, B, H, W, seed = 'MiT-B0', 'SegFormerHead', 19, 2, 64, 64, 3
    sd = OW.make_state_dict(backbone, head, nc, seed)
    x, y = OW.synthetic_batch(B, H, W, nc, seed)
    x, y = x.cuda(), y.cuda()
    args = types.SimpleNamespace(opt='sgd', lr=1e-3, momentum=0.9, weight_decay=0.025, opt_eps=None, opt_betas=None, head_lr_mult=10.0,
                                 layer_decay=None)

    def loss_fn(model, img, lbl):
        return criterion_lowres(model.forward_lowres(img), lbl, (H, W), None, num_classes=nc, dice=True, ignore_index=255)

    def build():
        m = SegmentationModel(backbone, num_classes=nc, seg_head=head, compute_dtype=torch.float32)
        m.load_state_dict(sd)
        m = m.cuda().train()
        for mod in m.backbone.modules():
            if hasattr(mod, 'drop_prob'):
                mod.drop_prob = 0.0
        m.decode_head.dropout.p = 0.0
        return m

    curves, kernels = [], []
    for graphed in (False, True):
        model = build()
        opt = create_optimizer(args, model)
        assert [pg['lr'] for pg in opt.param_groups] == [1e-3, 1e-3, 1e-2, 1e-2]
        losses = []
        if graphed:
            gs = GraphedTrainStep(model, opt, loss_fn, (x, y), clip_grad=1.0, clip_mode='norm', warmup=1)
            for _ in range(3):
                with hip.trace() as t:
                    losses.append(gs.step(x, y).item())
                kernels.append(t.kernels)
        else:
            scaler = NativeScaler()
            for _ in range(3):
                opt.zero_grad(set_to_none=True)
                loss = loss_fn(model, x, y)
                losses.append(loss.item())
                scaler(loss, opt, clip_grad=1.0, clip_mode='norm', parameters=model.parameters())
        curves.append(losses)
    print('eager', curves[0], 'graphed', curves[1])
    assert curves[0][0] != curves[0][-1]                       # the optimizer actually moved the loss
    assert all(any('flat_optim_groups_kernel' in n for n in k) for k in kernels), kernels
    np.testing.assert_allclose(curves[1], curves[0], rtol=2e-5)


def test_raw_entry_points_refuse_bad_group_tables():
    """ngroups 0, ngroups 129 and a null table: the error status, nothing launched, nothing changed."""
    from segmentation_factory_amd import hip
    lib = hip.lib()
    n = 40
    p, gr, s0, s1 = (torch.randn(n, device='cuda') for _ in range(4))
    s1.abs_()
    off = torch.tensor([0, 8, 16, 24, 32], dtype=torch.int64, device='cuda')
    ln = torch.full((5,), 8, dtype=torch.int32, device='cuda')
    flags = torch.zeros(5, dtype=torch.uint8, device='cuda')
    ug = torch.zeros(5, dtype=torch.uint8, device='cuda')
    ustep = torch.zeros(5, dtype=torch.int32, device='cuda')
    keep = [t.clone() for t in (p, s0, s1, ustep)]
    table = (C.c_float * 129)(*([1e-2] * 129))
    ptr = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    cases = [(0, table, table, ug), (129, table, table, ug), (-1, table, table, ug), (2, None, table, ug), (2, table, None, ug),
             (2, table, table, None)]
    with hip.trace() as t:
        for ngroups, lrs, wds, group in cases:
            dev = None if group is None else ptr(group)
            rc = lib.segf_agc_adamw_groups(ptr(p), ptr(gr), ptr(s0), ptr(s1), ptr(off), ptr(ln), ptr(flags), ptr(ustep), 5, dev,
                                           ngroups, lrs, wds, 0.9, 0.999, 1e-8, 1, 0.0, 1e-3, stream)
            assert rc == hip.ERR_SHAPE, (ngroups, rc)
            for rule in (0, 1, 2):
                rc = lib.segf_flat_optim_step_groups(rule, ptr(p), ptr(gr), ptr(s0), ptr(s1), ptr(off), ptr(ln), ptr(flags), ptr(ustep),
                                                     5, dev, ngroups, lrs, wds, 0.9, 0.9, 1e-8, 0, 0.0, 1e-3, stream)
                assert rc == hip.ERR_SHAPE, (rule, ngroups, rc)
        # each rule's own null-buffer rules hold in the group form too
        assert lib.segf_flat_optim_step_groups(1, ptr(p), ptr(gr), ptr(s0), None, ptr(off), ptr(ln), ptr(flags), ptr(ustep), 5, ptr(ug),
                                               2, table, table, 0.9, 0.9, 1e-8, 0, 0.0, 1e-3, stream) == hip.ERR_SHAPE
        assert lib.segf_flat_optim_step_groups(7, ptr(p), ptr(gr), ptr(s0), ptr(s1), ptr(off), ptr(ln), ptr(flags), ptr(ustep), 5,
                                               ptr(ug), 2, table, table, 0.9, 0.9, 1e-8, 0, 0.0, 1e-3, stream) == hip.ERR_SHAPE
    torch.cuda.synchronize()
    assert t.launches == 0 and t.kernels == []
    for a, b in zip((p, s0, s1, ustep), keep):
        assert torch.equal(a, b)
    with hip.trace() as t:                                     # and the call they refuse is a good one otherwise
        assert lib.segf_flat_optim_step_groups(0, ptr(p), ptr(gr), ptr(s0), None, ptr(off), ptr(ln), ptr(flags), None, 5, ptr(ug), 128,
                                               table, table, 0.9, 0.0, 0.0, 0, 0.0, 1e-3, stream) == 0
    assert t.launches == 1 and not torch.equal(p, keep[0])
