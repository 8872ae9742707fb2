"""Optimizer side of the train step: what engine.py:52-53 calls through timm 0.9.2 in the reference
(``loss_scaler(loss, optimizer, clip_grad=0.02, clip_mode='agc', parameters=..., create_graph=...)``).

timm is not available in the build image and no reference test covers this arithmetic, so AGC / AdamW are
restated from timm 0.9.2 + torch.optim.AdamW semantics ("parity unpinned") and checked against
the CPU restatement oracle/optim.py (tests/test_kernels_gpu.py::test_agc_adamw_known_answers).  The step itself is one HIP kernel over flat buffers.

The other --opt values (train_gpu.py:93-104,269: sgd / nesterov / momentum / adam / rmsprop) run on the same flat buffers through
segf_flat_optim_step.  Their ARITHMETIC is pinned: each rule is compared step for step with the torch.optim class of its name, which
is installed (tests/test_optimizers_gpu.py).  The mapping from the --opt NAME to a class and its arguments is restated from timm
0.9.2's create_optimizer_v2 and, like AGC, unpinned: timm is not available to compare against.

Parameter groups may carry their own lr and weight_decay: the step is then the group form of the same kernels (segf_agc_adamw_groups /
segf_flat_optim_step_groups: each unit looks its group's values up in a table that is a by-value kernel argument), pinned to torch.optim
with the same groups (tests/test_optim_groups_gpu.py).  --head-lr-mult and --layer-decay build such groups (param_groups_lr_scale;
the latter restates timm 0.9.2's param_groups_layer_decay: restated, not pinned).
"""
import torch

from . import hip


def _same(v):
    return tuple(v) if isinstance(v, (list, tuple)) else v


class FusedFlatOptimizer(torch.optim.Optimizer):
    """What every fused optimizer of this package shares: parameters re-homed into one flat fp32 buffer (each ``p.data`` becomes a
    view), gradients in a flat buffer of the same layout (gathered, or written in place by the backward formulas), the unit tables
    of the step kernels (one unit = one dim-0 row of a >=2-D weight or a whole 1-D tensor), the per-step "no gradient" flags, the
    per-unit step counts on the device, clipping in front of / inside the step, and a state_dict in the layout of the torch.optim
    class the subclass restates (RULE).  A subclass supplies its state buffers (_state_spec) and the kernel launch (apply_flat)."""
    FLAT_SLACK = 1024        # elements of zero padding behind the flat buffers (collective ranges round up to world x 16, graph.py)
    PARAM_ALIGN = 8          # every parameter starts at a multiple of this many elements in the flat buffers (_build)
    RULE = None              # name of the torch.optim class whose arithmetic and state_dict layout the subclass keeps
    SHARED = ()              # hyper-parameters that are launch scalars of the one kernel: every group must agree on them
    MAX_GROUPS = hip.OPT_MAX_GROUPS      # lr and weight_decay are per group: a table of this many entries is a kernel argument
    HAS_STEP = True          # the torch class keeps a per-parameter state['step']
    FIXED = {}               # group entries of the torch class that the kernel supports at one value only

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._flat = None
        self.direct = False
        self._step = 0
        self.agc_clip = 0.0          # set per step by NativeScaler when clip_mode == 'agc'
        self.force_groups = False    # tests / tools: take the group form of the step kernel even where the scalar form would do

    def add_param_group(self, param_group):
        if getattr(self, '_flat', None) is not None:
            raise RuntimeError(f'{type(self).__name__}.add_param_group: the flat buffers are built; their layout and the unit tables '
                               'of the step kernel are fixed by the groups that existed then')
        if len(self.param_groups) >= self.MAX_GROUPS:
            raise ValueError(f'{type(self).__name__}: at most {self.MAX_GROUPS} parameter groups (SEGF_OPT_MAX_GROUPS: the per-group '
                             'learning rates and weight decays are a fixed-size argument of the step kernel)')
        super().add_param_group(param_group)

    def _state_spec(self, group):
        """[(state_dict key, attribute holding the flat state buffer)] under the hyper-parameters of `group`."""
        raise NotImplementedError

    def _alloc_state(self):
        for _, attr in self._state_spec(self.param_groups[0]):
            if getattr(self, attr, None) is None:
                setattr(self, attr, torch.zeros_like(self._flat))

    def _build(self, order=None):
        """order: optional sequence of parameters (e.g. ``list(model.parameters())``) that fixes the LAYOUT of the flat buffers
        (registration order = reverse of the order in which backward finishes the gradients, so a suffix of the buffer is a
        bucket that completes early); default: parameter-group order.  The layout does not affect the arithmetic."""
        ps, decay, group_of = [], {}, {}
        for gi, g in enumerate(self.param_groups):
            for p in g['params']:
                if p.requires_grad:
                    ps.append(p)
                    decay[id(p)] = g['weight_decay'] > 0
                    group_of[id(p)] = gi
        if order is not None:
            rank = {id(p): i for i, p in enumerate(order)}
            ps.sort(key=lambda p: rank.get(id(p), len(rank)))
        dev = ps[0].device
        # every parameter starts on a PARAM_ALIGN-element boundary of the flat buffers (32 bytes in fp32, 16 bytes in the bf16 weight
        # shadow), whatever the sizes before it (a 19- or 171-class bias): the vector loads of the kernels that read weights in
        # place rely on it.  The gap elements stay zero in all four buffers and belong to no optimizer unit.
        self._spans = [-(-p.numel() // self.PARAM_ALIGN) * self.PARAM_ALIGN for p in ps]
        total = sum(self._spans)
        store = torch.zeros(total + self.FLAT_SLACK, dtype=torch.float32, device=dev)
        flat = store[:total]
        offs, lens, flags, ugroup = [], [], [], []
        o = 0
        for p, span in zip(ps, self._spans):
            d = decay[id(p)]
            n = p.numel()
            flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = flat[o:o + n].view(p.shape)
            rows = p.shape[0] if p.ndim > 1 else 1
            cols = n // rows
            for r in range(rows):
                offs.append(o + r * cols)
                lens.append(cols)
                flags.append(1 if d else 0)
                ugroup.append(group_of[id(p)])
            o += span
        self._params = ps
        self._flat = flat
        self._grad_store = torch.zeros(total + self.FLAT_SLACK, dtype=torch.float32, device=dev)
        self._grad = self._grad_store[:total]
        self._grad_views, self._offsets, o = [], [], 0
        for p, span in zip(ps, self._spans):
            self._grad_views.append(self._grad[o:o + p.numel()].view(p.shape))
            self._offsets.append(o)
            o += span
        self._alloc_state()
        self._off = torch.tensor(offs, dtype=torch.int64, device=dev)
        self._len = torch.tensor(lens, dtype=torch.int32, device=dev)
        self._flags = torch.tensor(flags, dtype=torch.uint8, device=dev)
        self._ugroup = torch.tensor(ugroup, dtype=torch.uint8, device=dev)      # each unit's parameter group (the group form of the step)
        # units (rows) of every parameter, for the per-step "received no gradient" bit (flag bit 1): torch.optim.AdamW -- the
        # reference's optimizer, train_gpu.py:269 -- skips a parameter whose .grad is None entirely (no decay, no moment update)
        self._unit_range, u = [], 0
        for p in ps:
            rows = p.shape[0] if p.ndim > 1 else 1
            self._unit_range.append((u, u + rows))
            u += rows
        self._base_flags = list(flags)
        self._nograd = frozenset()          # indices (into self._params) of parameters skipped by the current flags
        self._ustep = torch.zeros(len(flags), dtype=torch.int32, device=dev)   # per-unit step counts (torch's per-parameter state['step'])
        self._written = {}                  # direct placement: gradient-slot pointer -> deliveries in the current backward
        self.direct = False

    def _set_nograd(self, idx):
        """Mark the parameters `idx` (indices into the flat layout) as 'no gradient this step': the kernel leaves their
        parameters and moments untouched.  The flag tensor is rewritten only when the set changes."""
        idx = frozenset(idx)
        if idx == self._nograd:
            return
        flags = list(self._base_flags)
        for i in idx:
            lo, hi = self._unit_range[i]
            for u in range(lo, hi):
                flags[u] |= 2
        self._flags.copy_(torch.tensor(flags, dtype=torch.uint8), non_blocking=False)
        self._nograd = idx

    def set_clipping(self, clip_grad, clip_mode):
        """timm.utils.dispatch_clip_grad(parameters, value=clip_grad, mode=clip_mode) as part of the optimizer step: 'agc' inside
        the step kernel, 'norm' / 'value' as kernels over the flat gradient buffer right before it (segf_clip_grad)."""
        if clip_grad is not None and clip_mode not in ('agc', 'norm', 'value'):
            raise AssertionError(f"Unknown clip mode ({clip_mode}).")          # timm's wording
        self.clip_mode = clip_mode if clip_grad is not None else 'agc'
        self.clip_value = None if clip_grad is None else float(clip_grad)
        self.agc_clip = float(clip_grad) if (clip_grad is not None and clip_mode == 'agc') else 0.0

    def ensure_built(self, order=None):
        if self._flat is None:
            self._build(order)

    @property
    def flat_params(self):
        self.ensure_built()
        return self._flat

    @property
    def flat_grads(self):
        self.ensure_built()
        return self._grad

    @property
    def flat_grads_padded(self):
        """The gradient buffer including its FLAT_SLACK zero elements (collectives run over aligned ranges of this)."""
        self.ensure_built()
        return self._grad_store

    def enable_direct_grads(self, callback=None):
        """Hand every parameter its view of the flat gradient buffer (``p._segf_grad``): the backward formulas of
        segmentation_factory_amd.functional then write parameter gradients in place and ``.grad`` stays None
        (functional.direct_grads).  callback(view) is invoked, in backward order, whenever one gradient is final."""
        self.ensure_built()
        self._grad.zero_()
        self._user_cb = callback
        for p, view in zip(self._params, self._grad_views):
            p._segf_grad = view
            p._segf_grad_cb = self._note_delivery
            p.grad = None
        self.direct = True

    def begin_backward(self):
        """Direct placement: call before every forward+backward that is run from Python (warm-up, capture, eager steps)."""
        self._written = {}

    def _note_delivery(self, view):
        # a slot is an assignment target: a parameter consumed by two Functions in one step (tied weights, a module applied
        # twice) would keep only the last contribution and release its bucket early -- refuse instead of training on it
        k = view.data_ptr()
        if k in self._written:
            raise RuntimeError('direct gradient placement: a parameter received two gradients in one backward (tied weights / '
                               'a module applied twice); use the eager path (plain autograd accumulation) for such a model')
        self._written[k] = 1
        if self._user_cb is not None:
            self._user_cb(view)

    def finish_backward(self):
        """Direct placement: parameters that received neither an in-place gradient nor a .grad in the backward that just ran
        (e.g. FPNHead.output_convs[0], quirk Q3; frozen-by-construction plugin parts) are skipped by the optimizer kernel."""
        self._set_nograd(i for i, (p, v) in enumerate(zip(self._params, self._grad_views))
                         if v.data_ptr() not in self._written and p.grad is None)

    def disable_direct_grads(self):
        for p in getattr(self, '_params', []):
            for a in ('_segf_grad', '_segf_grad_cb'):
                if hasattr(p, a):
                    delattr(p, a)
        self.direct = False

    @torch.no_grad()
    def gather_grads(self):
        """Copy every parameter's .grad into the flat gradient buffer (multi-tensor copy; graph-capturable).  With direct
        placement only gradients that still arrived as ``.grad`` (foreign plugin modules on plain autograd) are copied."""
        self.ensure_built()
        dst, src, missing = [], [], []
        for i, (p, view) in enumerate(zip(self._params, self._grad_views)):
            if p.grad is not None:
                dst.append(view)
                src.append(p.grad)
            elif not self.direct:
                missing.append(i)
        if dst:
            torch._foreach_copy_(dst, src)
        if not self.direct:
            self._set_nograd(missing)          # torch.optim.AdamW: `if p.grad is None: continue`
            if missing and getattr(self, 'clip_mode', 'agc') in ('norm', 'value'):
                # clip_grad_norm_ / clip_grad_value_ ignore parameters without a gradient; the flat-buffer kernels see every slot, so a
                # gradient left over from an earlier step must not enter the global norm
                torch._foreach_zero_([self._grad_views[i] for i in missing])

    def _launch_scalars(self):
        """(first group, the one non-zero weight decay, per-group tables).  One kernel runs over the flat buffer.  The hyper-parameters in
        SHARED are its launch scalars, so every group must agree on them; anything else would be silently ignored.  lr and weight_decay
        are per group.  Decided per step from the groups' current values (a scheduler may make them differ later): where all groups share
        lr and the decays are {0, wd} (timm's param_groups_weight_decay) the tables are None and the step is the scalar kernel with
        weight decay as the on/off flag per unit; otherwise they are ([lr per group], [weight decay per group]) for the group form."""
        g, name = self.param_groups[0], type(self).__name__
        for pg in self.param_groups[1:]:
            if any(_same(pg[k]) != _same(g[k]) for k in self.SHARED):
                raise NotImplementedError(f'{name}: all parameter groups must share {" / ".join(self.SHARED)}')
        wds = {pg['weight_decay'] for pg in self.param_groups if pg['weight_decay'] > 0}
        tables = None
        if self.force_groups or len(wds) > 1 or any(pg['lr'] != g['lr'] for pg in self.param_groups[1:]):
            tables = ([float(pg['lr']) for pg in self.param_groups], [float(pg['weight_decay']) for pg in self.param_groups])
        return g, max(pg['weight_decay'] for pg in self.param_groups), tables

    def _clip_front(self):
        """Launch the 'norm' / 'value' clipping of the flat gradient buffer, if set; returns the AGC factor for the step kernel (0 = off)."""
        mode, value = getattr(self, 'clip_mode', 'agc'), getattr(self, 'clip_value', None)
        if mode in ('norm', 'value') and value is not None:      # timm dispatch_clip_grad's other modes, on the flat buffer
            if getattr(self, '_clip_ws', None) is None:
                self._clip_ws = torch.empty(int(hip.lib().segf_clip_grad_ws()), dtype=torch.float32, device=self._grad.device)
            hip.clip_grad(self._grad, mode, value, self._clip_ws)
        return float(self.agc_clip) if mode == 'agc' else 0.0

    def apply_flat(self):
        """The step over the flat buffers: one kernel launch of the subclass's rule."""
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        self.gather_grads()
        self.apply_flat()

    def _packed_ids(self):
        ids, i = {}, 0
        for g in self.param_groups:
            for p in g['params']:
                ids[id(p)] = i
                i += 1
        return ids

    def state_dict(self):
        """The state_dict layout of torch.optim.<RULE> (per-parameter entries under packed indices, only for parameters that have been
        stepped), so the checkpoint's 'optimizer_state' (train_gpu.py:354-362) can be read back by the torch class and vice versa."""
        sd = super().state_dict()
        if self._flat is not None and self._step > 0:
            ids = self._packed_ids()
            spec = self._state_spec(self.param_groups[0])
            state = {}
            usteps = self._ustep.cpu().tolist() if (spec or self.HAS_STEP) else None
            for i, p in enumerate(self._params if usteps is not None else []):
                n, o = p.numel(), self._offsets[i]
                t = usteps[self._unit_range[i][0]]
                if t > 0:                       # torch lists state only for parameters that have been stepped
                    st = {'step': torch.tensor(float(t))} if self.HAS_STEP else {}
                    for key, attr in spec:
                        st[key] = getattr(self, attr)[o:o + n].view(p.shape).detach().cpu().clone()
                    state[ids[id(p)]] = st
            sd['state'] = state
        return sd

    _RULE_OF_KEY = (('square_avg', 'RMSprop'), ('exp_avg', 'Adam / AdamW'), ('momentum_buffer', 'SGD'))

    def _check_loadable(self, groups, state):
        """Refuse, before anything is changed, a state_dict written by another rule: its moments would be dropped and training would
        continue on zeroed state without a word."""
        name = type(self).__name__
        missing = sorted(k for k in self.defaults if any(k not in g for g in groups))
        have = set().union(*(set(st) for st in state.values())) if state else set()
        theirs = next((r for k, r in self._RULE_OF_KEY if k in have), None)
        want = set() if missing else {k for k, _ in self._state_spec(groups[0])} | ({'step'} if self.HAS_STEP else set())
        if missing or any(st and not want <= set(st) for st in state.values()):
            raise ValueError(f'{name}.load_state_dict: this optimizer keeps torch.optim.{self.RULE} state, the state_dict holds '
                             + (f'{theirs} state ' if theirs else '') + f'({sorted(have)} per parameter'
                             + (f'; its groups lack {missing})' if missing else f', needed: {sorted(want)})'))
        for g in groups:
            for k, ok in self.FIXED.items():
                if g.get(k) is not None and g[k] != ok:
                    raise ValueError(f'{name}.load_state_dict: the state_dict was written with {k}={g[k]!r}; this kernel is '
                                     f'torch.optim.{self.RULE} with {k}={ok!r}')

    def load_state_dict(self, sd):
        """Accepts this class's own state_dict and one of torch.optim.<RULE> (the reference's checkpoints)."""
        sd = dict(sd)
        state = sd.get('state', {}) or {}
        self._check_loadable(sd['param_groups'], state)
        super().load_state_dict({'state': {}, 'param_groups': sd['param_groups']})
        if self._flat is not None:
            self._alloc_state()                 # the loaded groups may switch a state buffer on (momentum 0 -> 0.9)
        if not state:
            return
        self.ensure_built()
        by_index = {}
        for g in self.param_groups:
            for p in g['params']:
                by_index[len(by_index)] = p
        offs, pos = {}, {}
        for i, p in enumerate(self._params):
            offs[id(p)] = self._offsets[i]
            pos[id(p)] = i
        spec = self._state_spec(self.param_groups[0])
        for idx, st in state.items():
            p = by_index[int(idx)]
            if id(p) not in offs or not st:
                continue                        # frozen parameter: not part of the flat buffers
            o, n = offs[id(p)], p.numel()
            lo, hi = self._unit_range[pos[id(p)]]
            t = int(float(st['step'])) if 'step' in st else 1       # torch's SGD keeps no count: "has been stepped" is all that is known
            self._ustep[lo:hi] = t
            for key, attr in spec:
                if st[key] is not None:
                    getattr(self, attr)[o:o + n].copy_(st[key].reshape(-1))
            self._step = max(self._step, t)


class FusedAGCAdamW(FusedFlatOptimizer):
    """AdamW whose step (optionally preceded by unit-wise adaptive gradient clipping) runs as a single
    multi-tensor kernel (segf_agc_adamw).  Parameters are re-homed into one flat fp32 buffer (each
    ``p.data`` becomes a view), gradients are gathered into a flat buffer of the same layout."""
    RULE = 'AdamW'
    SHARED = ('betas', 'eps')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _state_spec(self, group):
        return [('exp_avg', '_m'), ('exp_avg_sq', '_v')]

    @torch.no_grad()
    def apply_flat(self):
        """AGC + AdamW over the flat buffers: one kernel launch (bias corrections are host scalars of this step)."""
        g, wd, tables = self._launch_scalars()
        self._step += 1
        agc = self._clip_front()
        if tables is None:
            hip.agc_adamw(self._flat, self._grad, self._m, self._v, self._off, self._len, self._flags, g['lr'], g['betas'][0],
                          g['betas'][1], g['eps'], wd, self._step, agc, unit_step=self._ustep)
        else:
            hip.agc_adamw_groups(self._flat, self._grad, self._m, self._v, self._off, self._len, self._flags, self._ugroup, *tables,
                                 g['betas'][0], g['betas'][1], g['eps'], self._step, agc, unit_step=self._ustep)

    def load_state_dict(self, sd):
        """Accepts this class's own state_dict and a torch.optim.AdamW / timm AdamW one (the reference's checkpoints)."""
        fused = dict(sd).get('fused', None)          # round-1 layout of this class
        if not (fused and fused.get('exp_avg') is not None):
            sd = dict(sd)
            sd.pop('fused', None)
            return super().load_state_dict(sd)
        torch.optim.Optimizer.load_state_dict(self, {'state': {}, 'param_groups': sd['param_groups']})
        self.ensure_built()
        self._step = int(fused['step'])
        self._ustep.fill_(self._step)
        # the round-1 layout was UNPADDED (parameters back to back); the flat buffers now align every parameter: scatter by offset
        m_old, v_old = fused['exp_avg'].reshape(-1), fused['exp_avg_sq'].reshape(-1)
        total = sum(p.numel() for p in self._params)
        if m_old.numel() == self._m.numel():               # written by a build with the same (padded) layout
            self._m.copy_(m_old)
            self._v.copy_(v_old)
        elif m_old.numel() == total:
            pos = 0
            for i, p in enumerate(self._params):
                n, o = p.numel(), self._offsets[i]
                self._m[o:o + n].copy_(m_old[pos:pos + n])
                self._v[o:o + n].copy_(v_old[pos:pos + n])
                pos += n
        else:
            raise ValueError(f"FusedAGCAdamW.load_state_dict: legacy 'fused' moments hold {m_old.numel()} values, the model has "
                             f'{total} parameters ({self._m.numel()} with alignment padding)')


class _FlatRuleOptimizer(FusedFlatOptimizer):
    """The rules of segf_flat_optim_step / segf_flat_optim_step_groups (csrc/optim.hip: flat_optim_kernel<RULE>, flat_optim_groups_kernel<RULE>).
    A subclass names its rule (KERNEL_RULE) and maps a group's hyper-parameters to (s0, s1, the rule's keyword arguments) in _rule_args."""

    @torch.no_grad()
    def apply_flat(self):
        g, wd, tables = self._launch_scalars()
        self._alloc_state()
        self._step += 1
        agc = self._clip_front()
        s0, s1, kw = self._rule_args(g, [getattr(self, attr) for _, attr in self._state_spec(g)])
        if tables is None:
            hip.flat_optim_step(self.KERNEL_RULE, self._flat, self._grad, s0, s1, self._off, self._len, self._flags, self._ustep, g['lr'],
                                wd, clip_factor=agc, **kw)
        else:
            hip.flat_optim_step_groups(self.KERNEL_RULE, self._flat, self._grad, s0, s1, self._off, self._len, self._flags, self._ustep,
                                       self._ugroup, *tables, clip_factor=agc, **kw)


class FusedSGD(_FlatRuleOptimizer):
    """torch.optim.SGD (momentum, optional Nesterov, dampening 0, weight decay coupled into the gradient) as one kernel over the
    flat buffers.  The momentum buffer starts at zero: torch clones the first gradient into it, which is momentum * 0 + g."""
    RULE = 'SGD'
    SHARED = ('momentum', 'nesterov')
    KERNEL_RULE = 'sgd'
    HAS_STEP = False
    FIXED = {'dampening': 0, 'maximize': False}

    def __init__(self, params, lr=1e-3, momentum=0, nesterov=False, weight_decay=0):
        if nesterov and momentum <= 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')          # torch's wording
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=nesterov))

    def _state_spec(self, group):
        return [('momentum_buffer', '_buf')] if group['momentum'] != 0 else []

    def _rule_args(self, g, bufs):
        return bufs[0] if bufs else None, None, dict(h0=g['momentum'], nesterov=g['nesterov'])


class FusedAdam(_FlatRuleOptimizer):
    """torch.optim.Adam: AdamW's moments with the weight decay coupled into the gradient (L2) instead of decoupled."""
    RULE = 'Adam'
    SHARED = ('betas', 'eps')
    FIXED = {'amsgrad': False, 'maximize': False, 'decoupled_weight_decay': False}
    KERNEL_RULE = 'adam'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _state_spec(self, group):
        return [('exp_avg', '_m'), ('exp_avg_sq', '_v')]

    def _rule_args(self, g, bufs):
        return bufs[0], bufs[1], dict(h0=g['betas'][0], h1=g['betas'][1], eps=g['eps'])


class FusedRMSprop(_FlatRuleOptimizer):
    """torch.optim.RMSprop (not centered), with its optional momentum buffer."""
    RULE = 'RMSprop'
    SHARED = ('alpha', 'eps', 'momentum')
    FIXED = {'centered': False, 'maximize': False}
    KERNEL_RULE = 'rmsprop'

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, momentum=0, weight_decay=0):
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, momentum=momentum, weight_decay=weight_decay, centered=False))

    def _state_spec(self, group):
        return [('square_avg', '_sq')] + ([('momentum_buffer', '_buf')] if group['momentum'] > 0 else [])

    def _rule_args(self, g, bufs):
        return bufs[0], bufs[1] if len(bufs) > 1 else None, dict(h0=g['alpha'], h1=g['momentum'], eps=g['eps'])


class NativeScaler:
    """Call-compatible stand-in for timm.utils.NativeScaler.  bf16 needs no loss scaling, so this is:
    backward -> (optional) clipping -> optimizer.step().  ``state_dict`` keeps the checkpoint key 'scaler'."""
    state_dict_key = 'amp_scaler'

    def __call__(self, loss, optimizer, clip_grad=None, clip_mode='norm', parameters=None, create_graph=False,
                 need_update=True):
        loss.backward(create_graph=create_graph)
        if not need_update:
            return
        if isinstance(optimizer, FusedFlatOptimizer):
            optimizer.set_clipping(clip_grad, clip_mode)
        elif clip_grad is not None:
            raise NotImplementedError('gradient clipping is fused into the FusedFlatOptimizer classes (FusedAGCAdamW, FusedSGD, '
                                      'FusedAdam, FusedRMSprop); use one of them or pass clip_grad=None')
        optimizer.step()

    def state_dict(self):
        return {}

    def load_state_dict(self, sd):
        pass


def param_groups_weight_decay(model, weight_decay):
    """timm.optim.optim_factory.param_groups_weight_decay: no decay for 1-D tensors and biases."""
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (no_decay if (p.ndim <= 1 or name.endswith('.bias')) else decay).append(p)
    return [{'params': no_decay, 'weight_decay': 0.}, {'params': decay, 'weight_decay': weight_decay}]


def param_groups_lr_scale(model, weight_decay, lr, head_lr_mult=1.0, layer_decay=None):
    """Parameter groups with their own learning rate: timm's two weight-decay groups split further by `lr_scale`.

    head_lr_mult M: parameters under ``decode_head.`` get lr_scale M (SegFormer's schedule trains the head at 10 x the backbone's
    rate): up to four groups.  layer_decay D: timm 0.9.2's param_groups_layer_decay restated, not pinned (timm is not installed):
    lr_scale = D ** (layer_max - layer_id) with a weight-decay and a no-decay group per layer; the layer ids of the backbone come from
    backbones.layer_id_map, everything outside ``backbone.`` (the decode head) sits at layer_max, scale 1.  Both together multiply.

    Every group carries 'lr_scale', 'lr' = lr * lr_scale (what the optimizer steps with until a scheduler writes the field) and
    'initial_lr' = lr, the schedulers' base value: they write value * lr_scale (scheduler.Schedule.update_groups), so the scale is
    applied once.  Groups are ordered by (layer, backbone before head, no-decay before decay); empty ones are left out."""
    ids, layer_max = None, 0
    if layer_decay is not None:
        from .backbones import layer_id_map
        ids = layer_id_map(model.backbone)
        layer_max = max(ids.values()) + 1
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        head = name.startswith('decode_head.')
        layer = layer_max
        if ids is not None and name.startswith('backbone.'):
            layer = ids[name[len('backbone.'):]]
        scale = (1.0 if layer_decay is None else float(layer_decay) ** (layer_max - layer)) * (float(head_lr_mult) if head else 1.0)
        decays = not (p.ndim <= 1 or name.endswith('.bias'))
        key = (layer, head, decays)
        if key not in groups:
            groups[key] = {'params': [], 'weight_decay': weight_decay if decays else 0., 'lr': lr * scale, 'lr_scale': scale,
                           'initial_lr': lr}
        groups[key]['params'].append(p)
    return [groups[k] for k in sorted(groups)]


OPT_NAMES = ('adam', 'adamw', 'momentum', 'nesterov', 'rmsprop', 'sgd')


def create_optimizer(args, model):
    """timm.optim.create_optimizer(args, model) (train_gpu.py:269) for the --opt values that have a fused kernel here: the branch of
    timm 0.9.2's create_optimizer_v2 that each name reaches, over timm's weight-decay groups (no decay for 1-D tensors and biases).
    The name -> class / argument mapping is restated, not pinned (timm is not installed); the arithmetic of every class is pinned to
    torch.optim.  `sgd` IS Nesterov in timm (`momentum` is the plain form); rmsprop gets alpha=0.9; the SGD forms drop --opt-eps.
    --head-lr-mult / --layer-decay (args.head_lr_mult, args.layer_decay) split those groups by learning rate (param_groups_lr_scale);
    with neither, the groups are exactly timm's two."""
    opt = str(getattr(args, 'opt', 'adamw')).lower()
    if opt not in OPT_NAMES:
        raise NotImplementedError(f"--opt {getattr(args, 'opt', None)}: the MI355X path has fused kernels for {', '.join(OPT_NAMES)} "
                                  "(the arithmetic of torch.optim's SGD / Adam / AdamW / RMSprop); timm's own optimizer classes are not implemented")
    wd = getattr(args, 'weight_decay', 0.025)
    lr, momentum = getattr(args, 'lr', 1e-3), getattr(args, 'momentum', 0.9)
    head_mult, layer_decay = getattr(args, 'head_lr_mult', 1.0), getattr(args, 'layer_decay', None)
    if head_mult == 1.0 and layer_decay is None:
        groups = param_groups_weight_decay(model, wd)
    else:       # --head-lr-mult / --layer-decay: groups with their own learning rate (the group form of the step kernels)
        groups = param_groups_lr_scale(model, wd, lr, 1.0 if head_mult is None else head_mult, layer_decay)
    eps = getattr(args, 'opt_eps', None)
    betas = getattr(args, 'opt_betas', None)
    if opt in ('sgd', 'nesterov'):
        return FusedSGD(groups, lr=lr, momentum=momentum, nesterov=True, weight_decay=wd)
    if opt == 'momentum':
        return FusedSGD(groups, lr=lr, momentum=momentum, nesterov=False, weight_decay=wd)
    if opt == 'rmsprop':
        return FusedRMSprop(groups, lr=lr, alpha=0.9, momentum=momentum, weight_decay=wd, **({} if eps is None else {'eps': eps}))
    if opt == 'adam':
        kw = {} if eps is None else {'eps': eps}
        if betas:
            kw['betas'] = tuple(betas)
        return FusedAdam(groups, lr=lr, weight_decay=wd, **kw)
    kw = dict(lr=lr, weight_decay=wd, eps=eps or 1e-8)
    if betas:
        kw['betas'] = tuple(betas)
    return FusedAGCAdamW(groups, **kw)
