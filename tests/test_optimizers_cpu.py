"""Host side of the --opt values beyond adamw (train_gpu.py:93-104,269): the name -> class mapping of create_optimizer (timm
0.9.2's create_optimizer_v2 restated; timm is not installed, so the mapping itself is unpinned) and the state_dict layout of
FusedSGD / FusedAdam / FusedRMSprop, which is that of the torch.optim class of the same rule.  No GPU: host tensors only."""
import types

import pytest
import torch

from segmentation_factory_amd import optim as O


def _args(opt, **kw):
    a = dict(opt=opt, lr=3e-3, weight_decay=0.05, momentum=0.8, opt_eps=1e-6, opt_betas=None)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _model():
    return torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3), torch.nn.Linear(3, 2))


@pytest.mark.parametrize('upper', [False, True])
def test_create_optimizer_name_mapping(upper):
    """Every supported --opt name, in either case, gives the class and arguments of timm 0.9.2's branch for it: `sgd` and `nesterov`
    are SGD WITH Nesterov momentum, `momentum` is the plain form, both without eps; rmsprop has alpha 0.9 and --momentum;
    adam / adamw take --opt-eps and --opt-betas.  Weight-decay groups are timm's: none for 1-D tensors and biases."""
    case = (lambda s: s.upper()) if upper else (lambda s: s)
    for name in ('sgd', 'nesterov', 'momentum'):
        o = O.create_optimizer(_args(case(name)), _model())
        assert type(o) is O.FusedSGD
        for g in o.param_groups:
            assert (g['lr'], g['momentum'], g['nesterov'], g['dampening']) == (3e-3, 0.8, name != 'momentum', 0) and 'eps' not in g
    o = O.create_optimizer(_args(case('rmsprop')), _model())
    assert type(o) is O.FusedRMSprop
    for g in o.param_groups:
        assert (g['lr'], g['alpha'], g['momentum'], g['eps'], g['centered']) == (3e-3, 0.9, 0.8, 1e-6, False)
    o = O.create_optimizer(_args(case('adam'), opt_betas=[0.8, 0.95]), _model())
    assert type(o) is O.FusedAdam
    for g in o.param_groups:
        assert (g['lr'], tuple(g['betas']), g['eps']) == (3e-3, (0.8, 0.95), 1e-6)
    assert tuple(O.create_optimizer(_args(case('adam')), _model()).param_groups[0]['betas']) == (0.9, 0.999)
    o = O.create_optimizer(_args(case('adamw')), _model())
    assert type(o) is O.FusedAGCAdamW and o.param_groups[0]['eps'] == 1e-6
    for o in (O.create_optimizer(_args(case(n)), _model()) for n in ('sgd', 'rmsprop', 'adam', 'adamw')):
        assert isinstance(o, O.FusedFlatOptimizer)
        assert [g['weight_decay'] for g in o.param_groups] == [0.0, 0.05]
        assert sorted(p.ndim for p in o.param_groups[0]['params']) == [1, 1, 1, 1] and [p.ndim for p in o.param_groups[1]['params']] == [2, 2]


def test_create_optimizer_refuses_other_names():
    with pytest.raises(NotImplementedError) as e:
        O.create_optimizer(_args('lamb'), _model())
    for name in ('sgd', 'nesterov', 'momentum', 'adam', 'adamw', 'rmsprop'):
        assert name in str(e.value)
    assert 'lamb' in str(e.value)
    with pytest.raises(ValueError):                     # torch's own refusal: Nesterov needs a momentum
        O.create_optimizer(_args('sgd', momentum=0.0), _model())


def _params(g):
    ps = [torch.nn.Parameter(torch.randn(4, 3, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g)),
          torch.nn.Parameter(torch.randn(2, 2, 3, generator=g))]
    ps[1].requires_grad_(False)                         # a frozen parameter keeps its packed index but has no state
    return ps


RULES = {
    'sgd_nesterov': (lambda ps: torch.optim.SGD(ps, lr=2e-4, momentum=0.9, nesterov=True, weight_decay=0.025),
                     lambda ps: O.FusedSGD(ps, lr=1.0, momentum=0.5), ['momentum_buffer'], '_buf'),
    'sgd_plain': (lambda ps: torch.optim.SGD(ps, lr=2e-4, weight_decay=0.025), lambda ps: O.FusedSGD(ps, lr=1.0, momentum=0.5), [], None),
    'adam': (lambda ps: torch.optim.Adam(ps, lr=2e-4, weight_decay=0.025), lambda ps: O.FusedAdam(ps, lr=1.0), ['step', 'exp_avg', 'exp_avg_sq'], '_v'),
    'rmsprop_momentum': (lambda ps: torch.optim.RMSprop(ps, lr=2e-4, alpha=0.9, momentum=0.9, weight_decay=0.025),
                         lambda ps: O.FusedRMSprop(ps, lr=1.0), ['step', 'square_avg', 'momentum_buffer'], '_buf'),
    'rmsprop_plain': (lambda ps: torch.optim.RMSprop(ps, lr=2e-4, alpha=0.9, weight_decay=0.025),
                      lambda ps: O.FusedRMSprop(ps, lr=1.0, momentum=0.9), ['step', 'square_avg'], '_sq'),
}


@pytest.mark.parametrize('rule', sorted(RULES))
def test_fused_state_dict_is_the_torch_class_layout(rule):
    """load_state_dict of the torch class's dict, state_dict(), and the torch class loads that back with equal tensors: the keys are
    those of the torch class (SGD: momentum_buffer only, nothing with momentum 0; Adam: step / exp_avg / exp_avg_sq; RMSprop: step /
    square_avg, plus momentum_buffer with momentum), under packed indices, none for the frozen parameter.  The hyper-parameters come
    from the loaded dict, including the ones that switch a state buffer on or off."""
    make_ref, make_fused, keys, last_attr = RULES[rule]
    g = torch.Generator().manual_seed(9)
    ps = _params(g)
    ref = make_ref(ps)
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g) if p.requires_grad else None
        ref.step()
    sd = ref.state_dict()
    fused = make_fused([torch.nn.Parameter(p.detach().clone(), requires_grad=p.requires_grad) for p in ps])
    fused.load_state_dict(sd)
    g0 = fused.param_groups[0]
    assert g0['lr'] == 2e-4 and g0['weight_decay'] == 0.025 and g0.get('momentum', 0) == ref.param_groups[0].get('momentum', 0)
    fused.ensure_built()                                # (a dict without state, SGD with momentum 0, leaves the buffers unbuilt)
    assert fused._offsets == [0, 16]                    # every parameter starts on a PARAM_ALIGN (8) boundary
    if last_attr:
        buf = getattr(fused, last_attr)
        assert buf.numel() == 32 and not buf[12:16].any()
        assert torch.equal(buf[16:28].view(2, 2, 3), sd['state'][2][keys[-1]])
    out = fused.state_dict()
    if not keys:
        assert out['state'] == {} and sd['state'] == {}
    else:
        assert set(out['state']) == {0, 2}
        for i in (0, 2):
            assert list(out['state'][i]) == keys
            for k in keys:
                assert torch.equal(torch.as_tensor(out['state'][i][k]), torch.as_tensor(sd['state'][i][k])), (i, k)
    back = make_ref(ps)
    back.load_state_dict(out)                           # torch accepts what we wrote ...
    for k in keys:
        assert torch.equal(torch.as_tensor(back.state[ps[0]][k]), torch.as_tensor(sd['state'][0][k]))
    for p in ps:                                        # ... and can step on it
        p.grad = torch.randn(p.shape, generator=g) if p.requires_grad else None
    back.step()
    if rule == 'sgd_nesterov':
        assert back.param_groups[0]['nesterov'] is True and back.param_groups[0]['dampening'] == 0


def test_state_of_another_rule_is_refused():
    """A checkpoint written under another --opt must not be read as 'no state yet': ValueError naming both rules, nothing changed."""
    g = torch.Generator().manual_seed(4)
    ps = _params(g)
    clone = lambda: [torch.nn.Parameter(p.detach().clone(), requires_grad=p.requires_grad) for p in ps]
    dicts = {}
    for name, make in (('AdamW', lambda q: torch.optim.AdamW(q, lr=1e-3)), ('SGD', lambda q: torch.optim.SGD(q, lr=1e-3, momentum=0.9)),
                       ('RMSprop', lambda q: torch.optim.RMSprop(q, lr=1e-3))):
        o = make(ps)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g) if p.requires_grad else None
        o.step()
        dicts[name] = o.state_dict()
    sgd = O.FusedSGD(clone(), lr=0.5, momentum=0.9)
    with pytest.raises(ValueError) as e:
        sgd.load_state_dict(dicts['AdamW'])
    assert 'SGD' in str(e.value) and 'AdamW' in str(e.value)
    assert sgd.param_groups[0]['lr'] == 0.5 and 'betas' not in sgd.param_groups[0]
    for fused, foreign in ((O.FusedSGD(clone(), lr=0.5, momentum=0.9), 'RMSprop'), (O.FusedAdam(clone()), 'SGD'),
                           (O.FusedRMSprop(clone()), 'AdamW'), (O.FusedAGCAdamW(clone()), 'SGD'), (O.FusedAdam(clone()), 'AdamW')):
        with pytest.raises(ValueError):
            fused.load_state_dict(dicts[foreign])
