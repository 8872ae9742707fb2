"""The --opt values beyond adamw (train_gpu.py:93-104,269) on the GPU: segf_flat_optim_step through FusedSGD / FusedAdam / FusedRMSprop
against the torch.optim class of the same rule run on the CPU, step for step -- with changing sets of gradient-less parameters, the
three --clip-mode values in front, a torch checkpoint continued, the step replayed as a hipGraph, and the CLI end to end.

Bars: max abs error < 2e-6 per step against torch (the project's bar for this comparison; on the inputs of the first test torch's own
fp32 run is within 4.2e-7 of its float64 run for every rule over the four steps), 1e-5 where AGC (restated in oracle/optim.py) is in
front, as tests/test_kernels_gpu.py::test_agc_adamw_known_answers."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 1e-2


def _rules():
    from segmentation_factory_amd.optim import FusedAdam, FusedRMSprop, FusedSGD
    return {
        'sgd': (lambda g: FusedSGD(g, lr=LR, momentum=0.9, nesterov=True), lambda g: torch.optim.SGD(g, lr=LR, momentum=0.9, nesterov=True)),
        'momentum': (lambda g: FusedSGD(g, lr=LR, momentum=0.9), lambda g: torch.optim.SGD(g, lr=LR, momentum=0.9)),
        'sgd_mu0': (lambda g: FusedSGD(g, lr=LR), lambda g: torch.optim.SGD(g, lr=LR)),
        'adam': (lambda g: FusedAdam(g, lr=LR), lambda g: torch.optim.Adam(g, lr=LR)),
        'rmsprop': (lambda g: FusedRMSprop(g, lr=LR, alpha=0.9, momentum=0.9), lambda g: torch.optim.RMSprop(g, lr=LR, alpha=0.9, momentum=0.9)),
        'rmsprop_mu0': (lambda g: FusedRMSprop(g, lr=LR, alpha=0.9), lambda g: torch.optim.RMSprop(g, lr=LR, alpha=0.9)),
    }


RULE_NAMES = ['sgd', 'momentum', 'sgd_mu0', 'adam', 'rmsprop', 'rmsprop_mu0']


def _groups(l, wd):
    return [{'params': [p for p in l if p.ndim <= 1], 'weight_decay': 0.}, {'params': [p for p in l if p.ndim > 1], 'weight_decay': wd}]


@pytest.mark.parametrize('rule', RULE_NAMES)
def test_fused_rule_matches_its_torch_class(rule):
    """Each rule against torch.optim on the CPU over four steps.  (3, 130): rows of two full lane strides plus a ragged tail of 2; the
    1-D tensors are single units; the 4-D tensor checks the row split.  Parameter 2 never gets a gradient: bit-equal, no state entry;
    parameter 1 misses one step and continues on its own count (Adam's bias corrections are per parameter in torch)."""
    make, make_ref = _rules()[rule]
    g = torch.Generator().manual_seed(3)
    shapes = [(5, 7), (5,), (4, 3, 2, 2), (9,), (3, 130)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in shapes]
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    opt, ropt = make(_groups(ps, 0.1)), make_ref(_groups(ref, 0.1))
    opt.set_clipping(None, 'agc')
    for step, have in enumerate([(0, 1, 3, 4), (0, 1, 3, 4), (0, 3, 4), (0, 1, 3, 4)]):
        for i, (p, r) in enumerate(zip(ps, ref)):
            if i in have:
                gr = torch.randn(*shapes[i], generator=g)
                p.grad, r.grad = gr.cuda(), gr.clone()
            else:
                p.grad, r.grad = None, None
        opt.step()
        ropt.step()
        errs = [(p.detach().cpu() - r.detach()).abs().max().item() for p, r in zip(ps, ref)]
        print(f'{rule} step {step}: max abs error per parameter {["%.2e" % e for e in errs]}')
        for i, e in enumerate(errs):
            assert e < 2e-6, (step, i, e)
    assert torch.equal(ps[2].detach().cpu(), ref[2].detach())         # untouched, bit for bit
    state = opt.state_dict()['state']
    rstate = ropt.state_dict()['state']
    assert set(state) == set(k for k, v in rstate.items() if v)      # packed indices; none for parameter 2 (index 3)
    assert 3 not in state and len(state) == (0 if rule == 'sgd_mu0' else 4)
    for k, st in state.items():
        assert set(st) == set(rstate[k])
        for name, v in st.items():       # the state buffers too: the same bar, relative to the buffer's largest entry where that exceeds 1
            want = torch.as_tensor(rstate[k][name]).float()
            assert (torch.as_tensor(v).float() - want).abs().max() <= 2e-6 * max(1.0, want.abs().max().item()), (k, name)
    if rule in ('adam', 'rmsprop'):
        assert float(state[0]['step']) == 3.0 and float(state[1]['step']) == 4.0     # parameter 1 (packed 0) counted its own steps


def _scaled_pair(rule, wd=0.05):
    make, make_ref = _rules()[rule]
    g = torch.Generator().manual_seed(5)
    shapes = [(6, 10), (6,), (3, 4, 2, 2), (17,)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in shapes]
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    return g, shapes, ps, ref, make(_groups(ps, wd)), make_ref(_groups(ref, wd))


@pytest.mark.parametrize('rule', ['sgd', 'rmsprop'])
@pytest.mark.parametrize('mode,value', [('norm', 0.5), ('norm', 1e4), ('value', 0.3)])
def test_clip_norm_and_value_in_front_of_the_rule(rule, mode, value):
    """--clip-mode norm / value through NativeScaler: the segf_clip_grad launches in front of the step, against torch's
    clip_grad_norm_ / clip_grad_value_ followed by the torch class's step."""
    from segmentation_factory_amd.optim import NativeScaler
    g, shapes, ps, ref, opt, ropt = _scaled_pair(rule)
    scaler = NativeScaler()
    for step in range(3):
        coefs = [torch.randn(*s, generator=g) * 2 for s in shapes]
        opt.zero_grad()
        scaler(sum((p * c.cuda()).sum() for p, c in zip(ps, coefs)), opt, clip_grad=value, clip_mode=mode, parameters=ps)
        ropt.zero_grad()
        sum((p * c).sum() for p, c in zip(ref, coefs)).backward()
        if mode == 'norm':
            torch.nn.utils.clip_grad_norm_(ref, value, norm_type=2.0)
        else:
            torch.nn.utils.clip_grad_value_(ref, value)
        ropt.step()
        for p, r in zip(ps, ref):
            err = (p.detach().cpu() - r.detach()).abs().max().item()
            print(f'{rule} {mode} {value} step {step}: max abs error {err:.2e}')
            assert err < 2e-6, (mode, step)


@pytest.mark.parametrize('rule', ['sgd', 'rmsprop'])
def test_agc_in_the_rule_kernel_clips_the_raw_gradient(rule):
    """--clip-mode agc (0.02) inside the step kernel against oracle.optim.adaptive_clip_grad_ on the gradient followed by the torch
    class's step.  Every unit of the weight-DECAYED group is clipped here (asserted), and the order matters: clipping g + wd * p
    instead of g -- the other order -- lands far outside the bar (asserted on the CPU), so the comparison shows that the kernel
    clips first and adds wd * p afterwards, as dispatch_clip_grad followed by optimizer.step() does."""
    from oracle import optim as OO
    from segmentation_factory_amd.optim import NativeScaler
    wd = 0.5
    g, shapes, ps, ref, opt, ropt = _scaled_pair(rule, wd)
    _, _, _, other, _, oopt = _scaled_pair(rule, 0.0)            # the wrong order, on the CPU: decay folded in before the clipping
    scaler = NativeScaler()
    for step in range(3):
        coefs = [torch.randn(*s, generator=g) * 2 for s in shapes]
        opt.zero_grad()
        scaler(sum((p * c.cuda()).sum() for p, c in zip(ps, coefs)), opt, clip_grad=0.02, clip_mode='agc', parameters=ps)
        for r, o, c in zip(ref, other, coefs):
            r.grad = OO.adaptive_clip_grad_(r.detach(), c.clone(), 0.02)
            if r.ndim > 1:
                assert not torch.equal(r.grad, c)                # the decayed group IS clipped
            o.grad = OO.adaptive_clip_grad_(o.detach(), c + (wd * o.detach() if o.ndim > 1 else 0), 0.02)
        ropt.step()
        oopt.step()
        for p, r in zip(ps, ref):
            err = (p.detach().cpu() - r.detach()).abs().max().item()
            print(f'{rule} agc step {step}: max abs error {err:.2e}')
            assert err < 1e-5, step
    assert max((r.detach() - o.detach()).abs().max().item() for r, o in zip(ref, other) if r.ndim > 1) > 1e-3


@pytest.mark.parametrize('rule', RULE_NAMES)
def test_fused_rule_continues_a_torch_checkpoint(rule):
    """Three steps of the torch class on the CPU, its state_dict loaded into the fused class: the next step on the GPU equals torch's."""
    make, make_ref = _rules()[rule]
    g = torch.Generator().manual_seed(21)
    shapes = [(6, 5), (7,), (3, 2, 3, 3), (4,)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    ref = make_ref([{'params': ps, 'weight_decay': 0.025}])
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    mine = [torch.nn.Parameter(p.detach().clone().cuda()) for p in ps]
    fused = make([{'params': mine}])
    fused.load_state_dict(ref.state_dict())
    assert fused.param_groups[0]['weight_decay'] == 0.025
    for p, q in zip(ps, mine):
        gr = torch.randn(p.shape, generator=g)
        p.grad, q.grad = gr.clone(), gr.clone().cuda()
    ref.step()
    fused.step()
    for p, q in zip(ps, mine):
        assert torch.allclose(q.detach().cpu(), p.detach(), rtol=2e-6, atol=1e-7)


def test_graphed_sgd_step_matches_eager_step():
    """GraphedTrainStep with FusedSGD (Nesterov, clip_mode='norm') walks the same loss curve as the eager sequence, and the engine
    chooses the graph for every fused class."""
    import types
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, criterion_lowres, engine
    from segmentation_factory_amd.graph import GraphedTrainStep
    from segmentation_factory_amd.optim import FusedAdam, FusedRMSprop, FusedSGD, NativeScaler, param_groups_weight_decay
    backbone, head, nc, B, H, W, seed = 'MiT-B0', 'SegFormerHead', 19, 2, 64, 64, 3
    sd = OW.make_state_dict(backbone, head, nc, seed)
    x, y = OW.synthetic_batch(B, H, W, nc, seed)
    x, y = x.cuda(), y.cuda()

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

    curves = []
    for graphed in (False, True):
        model = build()
        opt = FusedSGD(param_groups_weight_decay(model, 0.025), lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.025)
        losses = []
        if graphed:
            gs = GraphedTrainStep(model, opt, loss_fn, (x, y), clip_grad=1.0, clip_mode='norm', warmup=1)
            for _ in range(3):
                losses.append(gs.step(x, y).item())
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
    np.testing.assert_allclose(curves[1], curves[0], rtol=2e-5)
    args = types.SimpleNamespace(hip_graph=None)
    fresh = build()
    for o in (FusedSGD(fresh.parameters(), lr=1e-2, momentum=0.9, nesterov=True), FusedAdam(fresh.parameters()), FusedRMSprop(fresh.parameters())):
        assert engine._graph_step_wanted(args, fresh, fresh, o, NativeScaler(), 'cuda')
    assert not engine._graph_step_wanted(args, fresh, fresh, torch.optim.SGD(fresh.parameters(), lr=1e-2), NativeScaler(), 'cuda')


def test_train_gpu_cli_opt_sgd(tmp_path):
    """`train_gpu.py --opt sgd --momentum 0.9` end to end on generated data (one epoch of MiT-B0 + SegFormerHead at 64 x 64): the
    saved 'optimizer_state' is a torch.optim.SGD state_dict with Nesterov momentum (timm's `sgd`), and a second run resumes from it."""
    import subprocess
    import sys
    from segmentation_factory_amd import SegmentationModel
    from segmentation_factory_amd.optim import param_groups_weight_decay
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / 'out'
    cmd = [sys.executable, os.path.join(root, 'train_gpu.py'), '--dataset', 'synthetic', '--data_len', '8', '--image_size', '64',
           '--nb_classes', '5', '--backbone', 'MiT-B0', '--heads', 'SegFormerHead', '--batch-size', '2', '--val_batch_size', '2',
           '--epochs', '1', '--save_weights_dir', str(out), '--writer_output', str(tmp_path), '--train_print_freq', '1',
           '--val_print_freq', '1', '--lr', '1e-3', '--opt', 'sgd', '--momentum', '0.9']
    env = dict(os.environ, PYTHONPATH=root)
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Start training for 1 epochs' in r.stdout and 'train step captured as one hipGraph' in r.stdout, r.stdout[-2000:]
    ck = torch.load(str(out / 'MiT-B0_SegFormerHead_best_model.pth'), map_location='cpu', weights_only=False)
    model = SegmentationModel('MiT-B0', num_classes=5, seg_head='SegFormerHead')
    groups = param_groups_weight_decay(model, 0.025)
    sgd = torch.optim.SGD(groups, lr=1.0)
    sgd.load_state_dict(ck['optimizer_state'])
    assert all(g['nesterov'] is True and g['momentum'] == 0.9 and g['dampening'] == 0 for g in sgd.param_groups)
    packed = [p for g in groups for p in g['params']]
    state = ck['optimizer_state']['state']
    assert len(state) > 100
    for idx, st in state.items():
        assert list(st) == ['momentum_buffer'] and st['momentum_buffer'].shape == packed[idx].shape, idx
        assert torch.equal(sgd.state[packed[idx]]['momentum_buffer'], st['momentum_buffer'])
    r2 = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0 and 'Loading local checkpoint' in r2.stdout, r2.stdout[-2000:] + r2.stderr[-2000:]
