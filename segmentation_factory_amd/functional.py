"""Autograd operators over the HIP kernels (segmentation_factory_amd.hip).

Activations are token-major 2-D tensors ``[B*H*W, C]`` (NHWC flattened) in the compute dtype
(bf16 for speed, fp32 for the exact-parity mode); parameters and their gradients stay fp32.
Every forward/backward below is a hand-written formula over C-ABI kernel calls -- torch autograd
only sequences them.  Nothing here falls back to eager PyTorch math.
"""
import contextlib

import torch
from torch.autograd import Function

from . import hip


def _rowmajor(t):
    return t if t.stride(-1) == 1 else t.contiguous()


# bf16 shadow of the optimizer's flat parameter buffer (graph.GraphedTrainStep): inside `shadow_scope` a parameter that lives in
# the flat buffer is not cast per use -- the step casts the whole buffer with ONE launch at its start and `_w` hands out views
# (45 five-microsecond cast launches per SegFormer-B0 step otherwise).  Only active while the step function runs (warm-up,
# capture): outside, e.g. in evaluate() between epochs, the shadow would be one optimizer update behind.
_SHADOW = None


class shadow_scope:
    def __init__(self, table):
        self.table = table

    def __enter__(self):
        global _SHADOW
        self.prev, _SHADOW = _SHADOW, self.table
        return self

    def __exit__(self, *exc):
        global _SHADOW
        _SHADOW = self.prev
        return False


def _w(param, dtype):
    """fp32 master parameter -> compute dtype copy (bf16 cast kernel; identity in fp32 mode)."""
    p = param.detach()
    if _SHADOW is not None and dtype == torch.bfloat16 and p.is_contiguous():
        v = _SHADOW.get(p.data_ptr())
        if v is not None and v.numel() == p.numel():
            return v.view(p.shape)
    p = p if p.is_contiguous() else p.contiguous()
    return hip.cast(p, dtype) if dtype != torch.float32 else p


def _splitk(n_out, k_in, tokens):
    return hip.pick_splitk(n_out, k_in, tokens)


# ---- derived weight layouts ------------------------------------------------------------------------------------------------------
# Several layers consume a re-laid-out copy of a parameter (the [O][(ky,kx)][ci] matrix of a patch / spatial-reduction convolution,
# mit.py:105,47; the [49][C] table of a depthwise 7 x 7, convnext.py:29).  The copy depends on the weights alone, so inside a train
# step (graph.GraphedTrainStep) all of them are produced by ONE hip.prep_grouped launch at the start of the step instead of one launch
# in front of each layer: the registry learns the jobs during the first pass (where each still runs on its own) and replays them.
_DERIVED = None


class DerivedWeights:
    def __init__(self):
        self.entries = {}          # key -> (tensor handed to the layer, [prep jobs that (re)build it])
        self.fresh = False

    def refresh(self):
        jobs = [j for _, js in self.entries.values() for j in js]
        if jobs:
            hip.prep_grouped(jobs)
        self.fresh = True


@contextlib.contextmanager
def derived_scope(registry):
    """Inside: derived_weight() hands out the registry's copies, rebuilt here in one launch."""
    global _DERIVED
    prev = _DERIVED
    _DERIVED = registry
    try:
        if registry is not None:
            registry.refresh()
        yield
    finally:
        if registry is not None:
            registry.fresh = False
        _DERIVED = prev


def derived_weight(param, kind, make):
    """make() -> (tensor, jobs): allocate the derived copy and list the hip.prep_grouped jobs that fill it from `param`."""
    reg = _DERIVED
    key = (param.data_ptr(), kind)
    if reg is not None and reg.fresh:
        e = reg.entries.get(key)
        if e is not None:
            return e[0]
    t, jobs = make()
    hip.prep_grouped(jobs)
    if reg is not None:
        reg.entries[key] = (t, jobs)
    return t


def _tap_major(weight, dtype, kind, device):
    """The matrix [O][(ky,kx)][ci] of a convolution weight [O, Cin, kh, kw] in `dtype`, the operand of the products on im2col rows and of
    the implicit 3x3 GEMMs, as the derived weight `kind`; -> [O, taps * Cin]."""
    O, cin, taps = weight.shape[0], weight.shape[1], weight.shape[2] * weight.shape[3]
    wsrc = weight.detach().contiguous()

    def make():
        t = torch.empty((O, taps, cin), dtype=dtype, device=device)
        return t, [('perm', wsrc, t, O, cin, taps, cin)]
    return derived_weight(wsrc, kind, make).view(O, taps * cin)


def _tap_major_transposed(w, dtype):
    """[ci][(ky,kx)][co] from the 3x3 parameter [O, I, 3, 3]: the weight matrix of the implicit GEMM that forms the data gradient."""
    O, I = w.shape[0], w.shape[1]
    return hip.permute021(w.reshape(1, O, I * 9), 1, O, I * 9, dtype).view(I, 9 * O)


# ---- direct gradient placement ---------------------------------------------------------------------------------------------
# When the fused optimizer has re-homed the parameters into one flat buffer and `enable_direct_grads()` was called (the
# graphed train step does), every parameter carries `_segf_grad` = its fp32 view in the flat GRADIENT buffer.  The backward
# formulas below then write (or copy with segf_cast2d) the parameter gradients straight into those views and hand autograd
# `None`: no `.grad` tensors, no gather pass, no ATen accumulate / copy kernels inside the captured step, and the optimizer's
# `_segf_grad_cb` learns the moment a gradient is final (bucketed all-reduce overlapped with the rest of backward, graph.py).
def _slot(p):
    return getattr(p, '_segf_grad', None) if isinstance(p, torch.Tensor) else None


def _deliver_job(slot, value):
    """The copy job (hip.prep_grouped) that puts `value` into its flat-gradient view, or None when it already lives there."""
    if value is None or value.data_ptr() == slot.data_ptr():
        return None
    v = value.detach()
    assert v.dtype == torch.float32 and v.numel() == slot.numel(), (v.dtype, v.shape, slot.shape)
    if slot.ndim <= 1:                      # vectors (possibly a strided column of a wider buffer): copy as an [n, 1] matrix
        v, d = v.reshape(-1).unsqueeze(1), slot.reshape(-1).unsqueeze(1)
    else:
        v, d = v.reshape(slot.shape[0], -1), slot.reshape(slot.shape[0], -1)
        if v.stride(-1) != 1:
            v = v.contiguous()
    return ('cast', v, d)


def _deliver(slot_info, value):
    slot, cb = slot_info
    job = _deliver_job(slot, value)
    if job is not None:
        hip.cast2d(job[1], job[2])
    if cb is not None:
        cb(slot)


def _deliver_many(pairs):
    """[(slot_info, value)]: the copies of one backward formula's parameter gradients in ONE launch, then the delivery callbacks."""
    jobs = [j for j in (_deliver_job(info[0], v) for info, v in pairs) if j is not None]
    if len(jobs) == 1:
        hip.cast2d(jobs[0][1], jobs[0][2])
    elif jobs:
        hip.prep_grouped(jobs)
    for info, _ in pairs:
        if info[1] is not None:
            info[1](info[0])


# ---- deferred, grouped weight gradients -----------------------------------------------------------------------------------------
# The weight / bias gradients of the nn.Linear layers do not feed anything inside the backward pass, so under `defer_weight_grads()`
# (the captured train step) their dy^T x products are QUEUED by the backward formulas and issued together: hip.gemm_dw_db_grouped runs
# up to 12 layers per launch pair (csrc/gemm.hip: gemm_bf16_dw_group_kernel + splitk_reduce_group_kernel) instead of two launches per
# layer.  At the reference's default batch of 4 (train_gpu.py:71) those ~100 launches of 5 - 16 us were a quarter of the step.  Results
# are bitwise those of the per-layer launches; the queue keeps dy and x alive until the flush, and the direct-placement delivery
# callbacks (bucket events of the data-parallel exchange) fire at the flush.
_DW_QUEUE = None
DW_QUEUE_MAX = 12


_FIN_QUEUE = None          # deferred finalizes of two-stage column reductions (LayerNorm dgamma / dbeta), same scope
FIN_QUEUE_MAX = 32


def _flush_finalizes():
    q = _FIN_QUEUE
    if not q:
        return
    hip.colreduce_finalize_grouped([e[0] for e in q])
    for _, infos in q:
        for info in infos:
            _deliver(info, info[0])
    q.clear()


# dx of a LayerNorm whose input came out of a residual branch `x + DropPath(f(.))` (mit.py:143-146): the branch's backward starts by scaling
# that very gradient per sample (drop_path.py:18-25).  The LayerNorm backward kernel writes the scaled copy along with dx (one store more
# instead of a launch that reads dx again); it waits here, keyed by dx's address, for LinearFn.backward to pick it up.
_SCALED_DY = {}


def _park_scaled(dx, rscale, rpg):
    """dx.scaled (the DropPath-scaled copy a fused LayerNorm backward wrote) waits in _SCALED_DY for the backward of x's producer."""
    if getattr(dx, 'scaled', None) is not None:
        if len(_SCALED_DY) > 64:
            _SCALED_DY.clear()                   # (entries nobody came for: a consumer that did not need its input gradient)
        _SCALED_DY[dx.data_ptr()] = (dx.scaled, rscale.data_ptr(), rpg, dx._version)
        dx.scaled = None


def _scaled_dy(dy, rscale, rpg):
    """dy * rscale[row // rpg]: the copy parked by the LayerNorm backward that produced dy, when there was one, else a scale_rows launch."""
    hit = _SCALED_DY.pop(dy.data_ptr(), None)
    # hit[3]: dx's version when the entry was made.  The hand-over is only right while the tagged tensor has ONE consumer: a second
    # one makes autograd accumulate into dx in place (same address, version bumped) and the parked copy would be that of a partial sum
    if (hit is not None and hit[1] == rscale.data_ptr() and hit[2] == rpg and hit[0].shape == dy.shape and hit[0].dtype == dy.dtype
            and hit[3] == dy._version):
        return hit[0]
    return hip.scale_rows(dy, rscale, rpg)


def _adjacent_slots(ctx, i, j):
    """(slot of forward argument i, slot of j) when the two are ONE target in the flat gradient buffer, j's right behind i's, which a
    two-stage column reduction writes in place and whose finalize may be deferred; None otherwise."""
    a, b = gslot(ctx, i), gslot(ctx, j)
    if a is None or b is None or not a.is_contiguous() or b.data_ptr() != a.data_ptr() + 4 * a.numel():
        return None
    return a, b


def _queue_finalizes(ctx, *items):
    """items: (the finalize item a kernel called with defer=True left, the forward-argument positions whose slots it fills), for the scope's
    grouped finalize launch; the delivery callbacks of those slots fire at the flush."""
    q = _FIN_QUEUE
    for item, idx in items:
        q.append((item, tuple(ctx._gslots[i] for i in idx)))
    if len(q) >= FIN_QUEUE_MAX:
        _flush_finalizes()


def _ln_bwd(ctx, x, dy, g, mean, rstd, dy2=None, dres=None, dy2_patch=None):
    """LayerNorm backward with the (dgamma, dbeta) finalize deferred into the scope's grouped launch when both parameters carry adjacent
    flat-gradient slots; returns (dx, dgamma, dbeta) with None for gradients that will be delivered at the flush."""
    dgb = _adjacent_slots(ctx, 1, 2)
    dp = getattr(ctx, 'dp', None)
    rscale, rpg = dp if dp is not None else (None, 1)
    kw = dict(dgb_out=dgb, dy2=dy2, dres=dres, rscale=rscale, rows_per_group=rpg, dy2_patch=dy2_patch)
    if _FIN_QUEUE is not None and dgb is not None:
        dx, item = hip.layernorm_bwd(x, dy, g, mean, rstd, defer=True, **kw)
        _queue_finalizes(ctx, (item, (1, 2)))
        out = (dx, None, None)
    else:
        out = hip.layernorm_bwd(x, dy, g, mean, rstd, **kw)
    _park_scaled(out[0], rscale, rpg)
    return out


def flush_weight_grads():
    _flush_finalizes()
    q = _DW_QUEUE
    if not q:
        return
    # (the members' split-K counts were chosen per layer; inside a group they may share one smaller count: hip / segfac.h shared_split)
    hip.gemm_dw_db_grouped([e[0] for e in q], shared_split=not hip.policy('dw_no_shared_split'))
    # the layout passes behind the products (the [O][k k][Cin] -> OIHW permutes of the patch convolutions' weight gradients): one launch
    hip.prep_grouped([post for _, _, post in q if post is not None])
    for _, infos, post in q:
        for info in infos:
            _deliver(info, info[0])                   # the slot IS the result: no copy, only the delivery callback
    q.clear()


@contextlib.contextmanager
def defer_weight_grads():
    global _DW_QUEUE, _FIN_QUEUE
    prev, prevf = _DW_QUEUE, _FIN_QUEUE
    _DW_QUEUE = [] if not hip.policy('no_deferred_dw') else None
    _FIN_QUEUE = [] if not hip.policy('no_deferred_finalize') else None
    try:
        yield
        flush_weight_grads()
    finally:
        _DW_QUEUE, _FIN_QUEUE = prev, prevf
        _SCALED_DY.clear()          # entries nobody collected must not outlive the backward they belong to (their addresses get reused)


def _queue_dw(ctx, dy, x, n_out, n_in, tokens, iw=1, ib=2, post_of=None):
    """Queue dW [n_out, n_in] = dy^T x and db = colsum(dy) of a Linear whose parameters (forward arguments iw, ib) both carry flat-gradient
    slots; False when the product has to be issued by the caller (no scope, no slots).  post_of: the weight gradient needs a layout pass
    behind the product, which then lands in a temporary [n_out, n_in] fp32 matrix, and the hip.prep_grouped job
    post_of(temp, weight_slot) runs after the grouped launch."""
    q = _DW_QUEUE
    slots = getattr(ctx, '_gslots', None)
    if q is None or not slots or iw not in slots or ib not in slots:
        return False
    gw, gb = slots[iw][0], slots[ib][0]
    if gb.numel() != n_out or not gb.is_contiguous():
        return False
    if post_of is None:
        dst, post = gw.view(n_out, n_in), None
    else:
        dst = torch.empty((n_out, n_in), dtype=torch.float32, device=dy.device)
        post = post_of(dst, gw)
    q.append(((dy, x, n_out, n_in, tokens, _splitk(n_out, n_in, tokens), dst, gb), (slots[iw], slots[ib]), post))
    if len(q) >= DW_QUEUE_MAX:
        flush_weight_grads()
    return True


def _from_tap_major(dwm, n_out, taps, cin, out=None):
    """A convolution's weight gradient as its product leaves it, [O][(ky,kx)][ci] fp32, in the parameter's own [O][ci][(ky,kx)] layout;
    out: the flat-gradient slot to write."""
    return hip.permute021(dwm, n_out, taps, cin, torch.float32, out=out)


def _linear_param_grads(ctx, dy, x, n_out, n_in, tokens, iw, ib, has_bias, wshape, taps=None):
    """(dW, db) of a Linear-like layer y = x W^T + b whose weight and bias are the forward arguments iw, ib (ib None: no bias):
    dW = dy^T x [n_out, n_in] in fp32, viewed as `wshape`, and db = colsum(dy), each None when it is not wanted -- or when it will be
    delivered at the flush of defer_weight_grads().  Both wanted: queued for the scope's grouped launch where one is open and both
    parameters carry flat-gradient slots (_queue_dw), else one pass over dy for both (hip.gemm_dw_db); only one: its own product or
    column sum.  Whatever is issued here writes the parameter's flat-gradient slot where it has one.
    taps: the layer is a convolution on an im2col matrix and the product comes out [n_out][taps][n_in / taps]: it lands in a temporary
    and a layout pass (_from_tap_major, or its hip.prep_grouped job behind the grouped launch) writes the slot."""
    need_w, need_b = ctx.needs_input_grad[iw], has_bias and ctx.needs_input_grad[ib]
    gw, gb = gslot(ctx, iw), gslot(ctx, ib)
    out = post_of = None
    if taps is None:
        out = gw.view(n_out, n_in) if gw is not None else None
    else:
        cin = n_in // taps
        post_of = lambda t, g: ('perm', t, g, n_out, taps, cin, taps)       # noqa: E731
    dw = db = None
    if need_w and need_b:
        if _queue_dw(ctx, dy, x, n_out, n_in, tokens, iw, ib, post_of):           # deferred + grouped under defer_weight_grads(); else right here
            return None, None
        dw, db = hip.gemm_dw_db(dy, x, n_out, n_in, tokens, split_k=_splitk(n_out, n_in, tokens), out=out, db_out=gb)   # one pass over dy for both
    elif need_w:
        dw = hip.gemm(2, dy, x, n_out, n_in, tokens, out=out, out_dtype=torch.float32, split_k=_splitk(n_out, n_in, tokens))
    elif need_b:
        db = hip.colsum(dy, out=gb)
    if dw is not None:
        if taps is not None:
            dw = _from_tap_major(dw, n_out, taps, cin, out=gw)
        dw = dw.view(wshape)
    return dw, db


def direct_grads(*param_idx):
    """Class decorator for the autograd Functions: the gradients of the forward arguments at positions `param_idx` (parameters)
    go to the optimizer's flat gradient buffer when the parameter carries a `_segf_grad` view; a backward that already wrote
    into `ctx.gslot(i)` (e.g. as the `out=` of its GEMM) returns that view and no copy is made."""
    def deco(cls):
        fwd, bwd = cls.forward, cls.backward

        def forward(ctx, *args):
            slots = None
            for i in param_idx:
                if i < len(args):
                    sl = _slot(args[i])
                    if sl is not None:
                        if slots is None:
                            slots = {}
                        slots[i] = (sl, getattr(args[i], '_segf_grad_cb', None))
            ctx._gslots = slots
            return fwd(ctx, *args)

        def backward(ctx, *grads):
            out = bwd(ctx, *grads)
            slots = getattr(ctx, '_gslots', None)
            if not slots:
                return out
            out = list(out) if isinstance(out, tuple) else [out]
            pairs = [(info, out[i]) for i, info in slots.items() if out[i] is not None]
            _deliver_many(pairs)
            for i in slots:
                out[i] = None
            return tuple(out)
        cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
        return cls
    return deco


def gslot(ctx, i, shape=None):
    """The flat-buffer view for forward argument i (or None): pass it as `out=` to write the gradient in place."""
    slots = getattr(ctx, '_gslots', None)
    if not slots or i not in slots:
        return None
    v = slots[i][0]
    return v.view(shape) if shape is not None else v


def _padded_rows(weight, bias, N, Np, K, dtype, device):
    """(w [Np, K] in `dtype`, b [Np] fp32 or None): the layer's parameters with zero rows up to Np (a column-padded output, e.g. 150 classes
    -> 152).  Weights-only work: inside a train step it comes from the step's one derived-weights launch."""
    wsrc = weight.detach().reshape(N, -1)

    def make_w():
        t = torch.empty((Np, K), dtype=dtype, device=device)
        return t, [('cast', wsrc, t[:N]), ('zero', t[N:])]
    w = derived_weight(weight.detach(), ('padrows', dtype, Np), make_w)
    b = None
    if bias is not None:
        bsrc = bias.detach()

        def make_b():
            t = torch.empty((Np,), dtype=torch.float32, device=device)
            return t, [('cast', bsrc.unsqueeze(1), t[:N].unsqueeze(1)), ('zero', t[N:])]
        b = derived_weight(bsrc, ('padrows', Np), make_b)
    return w, b


@direct_grads(1, 2)
class LinearFn(Function):
    """y = [residual + rscale[b] *] (x W^T + bias)   (nn.Linear / 1x1 conv on tokens).
    reference: mit.py:45,52,58,98-99 (q/kv/proj/fc1/fc2), heads/segformer.py:13,24,39."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, rscale, rows_per_group, pad_to, fp8=False):
        x = _rowmajor(x)
        M, K = x.shape
        N = weight.shape[0]
        Np = pad_to if (pad_to and pad_to > N) else N
        if fp8 and Np == N and x.dtype == torch.bfloat16 and hip.linear_fp8_supported(0, M, N, K):
            # FP8 on the 256 x 256 tile kernel (BASELINE cfg5): the activation tensor quantised to e4m3 with ONE dynamic scale, the
            # weight rows with one each.  The quantised input is kept for the weight gradient (instead of the bf16 tensor, when that
            # product has an fp8 form too); the backward quantises the gradient once (e5m2) for its two products.
            w = _w(weight.reshape(N, -1), x.dtype)
            xq, sx = hip.quant_tensor_fp8(x)
            wq, sw = hip.quant_rows_fp8(weight.detach().reshape(N, -1))
            y = hip.linear_fp8(0, xq, sx, wq, sw, bias=bias.detach() if bias is not None else None, residual=residual, rscale=rscale,
                               rows_per_group=rows_per_group or 1)
            keep8 = hip.linear_fp8_supported(2, M, N, K)
            ctx.save_for_backward(None if keep8 else x, w, rscale, xq if keep8 else None, sx if keep8 else None)
            ctx.meta = (M, N, K, bias is not None, residual is not None, rows_per_group or 1, weight.shape, Np)
            ctx.fp8t = True
            return y
        if fp8 and Np == N and x.dtype == torch.bfloat16 and hip.gemm_fp8_supported(M, N, K):
            # FP8 forward (BASELINE cfg5): token rows and output-channel rows quantised to e4m3 with dynamic amax scales, product
            # on the block-scaled fp8 matrix instruction; the backward products below stay bf16 on the saved operands
            w = _w(weight.reshape(N, -1), x.dtype)
            xq, sx = hip.quant_rows_fp8(x)
            wq, sw = hip.quant_rows_fp8(weight.detach().reshape(N, -1))
            y = hip.gemm_fp8(xq, sx, wq, sw, bias=bias.detach() if bias is not None else None, residual=residual, rscale=rscale,
                             rows_per_group=rows_per_group or 1)
            ctx.save_for_backward(x, w, rscale)
            ctx.meta = (M, N, K, bias is not None, residual is not None, rows_per_group or 1, weight.shape, Np)
            return y
        if Np > N:
            # column-padded output (e.g. 150 classes -> 152): the layer is run as an Np-wide linear whose extra weight rows
            # and biases are zero, so the pad columns of y are exact zeros, every 16-byte chunk of a row is either fully
            # valid or fully padding, and the backward products take the padded gradient as it stands
            assert residual is None
            w, b = _padded_rows(weight, bias, N, Np, K, x.dtype, x.device)
            y = hip.gemm(0, x, w, M, Np, K, bias=b)[:, :N]
        else:
            w = _w(weight.reshape(N, -1), x.dtype)
            b = bias.detach() if bias is not None else None
            y = hip.gemm(0, x, w, M, N, K, bias=b, residual=residual, rscale=rscale, rows_per_group=rows_per_group or 1)
        ctx.save_for_backward(x, w, rscale)
        ctx.meta = (M, N, K, bias is not None, residual is not None, rows_per_group or 1, weight.shape, Np)
        return y

    @staticmethod
    def backward(ctx, dy):
        if getattr(ctx, 'fp8t', False):
            return LinearFn._backward_fp8(ctx, dy)
        x, w, rscale = ctx.saved_tensors
        M, N, K, has_bias, has_res, rpg, wshape, Np = ctx.meta
        dy = _rowmajor(dy)
        if Np > N and dy.stride(0) == Np:
            # the gradient arrives in a column-padded buffer; every kernel of this library that writes padded rows zero-fills
            # the pad (segfac.h), so the products run Np wide and the zero rows / columns are sliced away afterwards
            dyp = dy.as_strided((M, Np), (Np, 1))
            dx = hip.gemm(1, dyp, w, M, K, Np) if ctx.needs_input_grad[0] else None
            dw = db = None
            if ctx.needs_input_grad[1] and has_bias and ctx.needs_input_grad[2]:
                dw, db = hip.gemm_dw_db(dyp, x, Np, K, M, split_k=_splitk(Np, K, M))
                dw, db = dw[:N].view(wshape), db[:N]
            else:
                if ctx.needs_input_grad[1]:
                    dw = hip.gemm(2, dyp, x, Np, K, M, out_dtype=torch.float32, split_k=_splitk(Np, K, M))[:N].view(wshape)
                if has_bias and ctx.needs_input_grad[2]:
                    db = hip.colsum(dyp)[:N]
            return dx, dw, db, None, None, None, None, None
        wv = w[:N] if Np > N else w
        dys = _scaled_dy(dy, rscale, rpg) if rscale is not None else dy
        dx = hip.gemm(1, dys, wv, M, K, N) if ctx.needs_input_grad[0] else None
        dw, db = _linear_param_grads(ctx, dys, x, N, K, M, 1, 2, has_bias, wshape)
        dres = dy if (has_res and ctx.needs_input_grad[3]) else None
        return dx, dw, db, dres, None, None, None, None


def _linear_backward_fp8(ctx, dy):
    """Backward of the tensor-scaled fp8 Linear: dx = dy W and dW = dy^T x on fp8 operands where the shapes have the tile kernel
    (the gradient quantised once, e5m2, one scale), bf16 otherwise; the bias gradient is a column sum of the bf16 gradient."""
    x, w, rscale, xq, sx = ctx.saved_tensors
    M, N, K, has_bias, has_res, rpg, wshape, Np = ctx.meta
    dy = _rowmajor(dy)
    dys = hip.scale_rows(dy, rscale, rpg) if rscale is not None else dy
    dx8 = ctx.needs_input_grad[0] and hip.linear_fp8_supported(1, M, K, N)
    dw8 = ctx.needs_input_grad[1] and xq is not None
    gq = sg = None
    if dx8 or dw8:
        gq, sg = hip.quant_tensor_fp8(dys, e5m2=True)
    dx = dw = db = None
    if ctx.needs_input_grad[0]:
        if dx8:
            wt = hip.permute021(w.reshape(1, N, K), 1, N, K, w.dtype).view(K, N)       # W^T, rows = input features
            wtq, swt = hip.quant_rows_fp8(wt)
            dx = hip.linear_fp8(1, gq, sg, wtq, swt)
        else:
            dx = hip.gemm(1, dys, w, M, K, N)
    gw, gb = gslot(ctx, 1, (N, K)), gslot(ctx, 2)
    if ctx.needs_input_grad[1]:
        if dw8:
            dw = hip.linear_fp8_wgrad(gq, sg, xq, sx, out=gw).view(wshape)
        else:
            dw = hip.gemm(2, dys, x, N, K, M, out=gw, out_dtype=torch.float32, split_k=_splitk(N, K, M)).view(wshape)
    if has_bias and ctx.needs_input_grad[2]:
        db = hip.colsum(dys, out=gb)
    dres = dy if (has_res and ctx.needs_input_grad[3]) else None
    return dx, dw, db, dres, None, None, None, None


LinearFn._backward_fp8 = staticmethod(_linear_backward_fp8)


@direct_grads(1, 2)
class LinearForkFn(Function):
    """(y, x') = (x W^T + bias, x): a Linear whose input has a second consumer (MiT attention: q = Linear(h) while h also feeds
    the key / value path, mit.py:52-53).  The second consumer's gradient arrives as an argument of this backward and rides into
    the data-gradient product as its residual operand, dx = dx' + dy W, instead of a separate add launch per block."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = _rowmajor(x)
        M, K = x.shape
        N = weight.shape[0]
        w = _w(weight.reshape(N, -1), x.dtype)
        y = hip.gemm(0, x, w, M, N, K, bias=bias.detach() if bias is not None else None)
        ctx.save_for_backward(x, w)
        ctx.meta = (M, N, K, bias is not None, weight.shape)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dx2):
        x, w = ctx.saved_tensors
        M, N, K, has_bias, wshape = ctx.meta
        dy = _rowmajor(dy)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = hip.gemm(1, dy, w, M, K, N, residual=_rowmajor(dx2) if dx2 is not None else None)
        dw, db = _linear_param_grads(ctx, dy, x, N, K, M, 1, 2, has_bias, wshape)
        return dx, dw, db


def linear_fork(x, weight, bias=None):
    """(Linear(x), alias of x for a second consumer) -- see LinearForkFn"""
    return LinearForkFn.apply(x, weight, bias)


def linear(x, weight, bias=None, residual=None, rscale=None, rows_per_group=None, pad_to=None, fp8=False):
    y = LinearFn.apply(x, weight, bias, residual, rscale, rows_per_group, pad_to, fp8)
    if rscale is not None and not fp8:
        y._segf_dp = (rscale, rows_per_group or 1)         # a LayerNorm that consumes y can prepare this layer's scaled gradient (_ln_bwd)
    return y


def _ln_enter(ctx, x, gamma, beta, dp_scale, dp_rpg, patch=None):
    """Forward entry of the LayerNorm family: ctx.dp = the DropPath hand-over of x's producer (_dp_of) for the backward, ctx.patch = the
    (log2 W, log2 sr) of a patch-major second output; -> (x, gamma, beta) as the kernels take them."""
    ctx.dp = (dp_scale, int(dp_rpg)) if dp_scale is not None else None
    if patch is not None:
        ctx.patch = (int(patch[0]), int(patch[1]))
    x = x if x.is_contiguous() else x.contiguous()
    return x, gamma.detach().contiguous(), beta.detach().contiguous()


@direct_grads(1, 2)
class LayerNormFn(Function):
    """nn.LayerNorm over the channel dim of token rows (mit.py:107,136-140; convnext.py:8-23 in NHWC)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, dp_scale=None, dp_rpg=1):
        x, g, b = _ln_enter(ctx, x, gamma, beta, dp_scale, dp_rpg)
        y, mean, rstd = hip.layernorm_fwd(x, g, b, eps)
        ctx.save_for_backward(x, g, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, mean, rstd = ctx.saved_tensors
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dx, dg, db = _ln_bwd(ctx, x, dy, g, mean, rstd)       # adjacent flat-gradient views are one [2][C] target, written in place
        return dx, dg, db, None, None, None


def _dp_of(x):
    """(rscale, rows_per_group) when x is the output of a `residual + DropPath-scaled branch` product (functional.linear tags it)"""
    dp = getattr(x, '_segf_dp', None)
    return dp if dp is not None and not hip.policy('no_scaled_ln_bwd') else (None, 1)


def layer_norm(x, gamma, beta, eps):
    return LayerNormFn.apply(x, gamma, beta, eps, *_dp_of(x))


@direct_grads(1, 2)
class LayerNormResFn(Function):
    """The pre-norm residual pattern `x + f(norm(x))` (mit.py:143-146, convnext.py:36-50): returns (x, norm(x)) -- x passes
    through for the residual add -- so that the backward sees BOTH gradients of x at once and the LayerNorm backward kernel adds
    the residual-path gradient while it stores dx (no separate gradient-accumulation kernel)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, dp_scale=None, dp_rpg=1):
        x, g, b = _ln_enter(ctx, x, gamma, beta, dp_scale, dp_rpg)
        y, mean, rstd = hip.layernorm_fwd(x, g, b, eps)
        ctx.save_for_backward(x, g, mean, rstd)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, dres, dy):
        x, g, mean, rstd = ctx.saved_tensors
        if dy is None:
            return dres, None, None, None, None, None
        dy = dy if dy.is_contiguous() else dy.contiguous()
        if dres is not None and not dres.is_contiguous():
            dres = dres.contiguous()
        dx, dg, db = _ln_bwd(ctx, x, dy, g, mean, rstd, dres=dres)
        return dx, dg, db, None, None, None


def layer_norm_res(x, gamma, beta, eps):
    """-> (x, LayerNorm(x)): use the returned x for the residual connection."""
    return LayerNormResFn.apply(x, gamma, beta, eps, *_dp_of(x))


def _ln_linear_fwd_fused(x, g, b, w, bias):
    """May the forward of Linear(LayerNorm(x)) run as hip.layernorm_linear_fwd?  The library's rule (SEGFAC_LN_LINEAR_FWD_FUSED) and the
    16-byte alignment its vector loads of the parameters need."""
    return (bias is not None and bias.dtype == torch.float32 and hip.layernorm_linear_fwd_supported(x.dtype, x.shape[0], x.shape[1], w.shape[0])
            and all(t.data_ptr() % 16 == 0 for t in (x, g, b, w)) and bias.data_ptr() % 4 == 0)


def _ln_linear_bwd(ctx, dh, dres, x, g, b, mean, rstd, y, w, iw, ib, dy2=None, dy2_patch=None):
    """hip.layernorm_linear_bwd for a formula whose forward arguments 1, 2 are the norm's parameters and iw, ib the Linear's: the four
    parameter gradients written in place / deferred into the scope's grouped finalize where all four carry flat-gradient slots.
    -> (dx, dgamma, dbeta, dw, dbias) with None for gradients that are delivered at the flush."""
    N, K = w.shape
    rscale, rpg = ctx.dp if ctx.dp is not None else (None, 1)
    dgb, gw, gb1 = _adjacent_slots(ctx, 1, 2), gslot(ctx, iw), gslot(ctx, ib)
    outs = None
    if dgb is not None and gw is not None and gb1 is not None and gw.is_contiguous() and gb1.is_contiguous():
        outs = (gw.view(N, K), gb1, *dgb)
    kw = dict(dres=dres, rscale=rscale, rows_per_group=rpg, outs=outs)
    if y is None:
        kw.update(beta=b, dy2=dy2, dy2_patch=dy2_patch)
    if _FIN_QUEUE is not None and outs is not None:
        dx, items = hip.layernorm_linear_bwd(dh, w, x, y, g, mean, rstd, defer=True, **kw)
        _queue_finalizes(ctx, (items[0], (iw,)), (items[1], (ib,)), (items[2], (1, 2)))
        res = (dx, None, None, None, None)
    else:
        dx, dw, db1, dg, db = hip.layernorm_linear_bwd(dh, w, x, y, g, mean, rstd, **kw)
        res = (dx, dg, db, dw.view(ctx.wshape), db1)
    _park_scaled(dx, rscale, rpg)                 # parked for the backward of x's producer, as _ln_bwd parks it
    return res


@direct_grads(1, 2, 4, 5)
class LayerNormResLinearFn(Function):
    """(x, Linear(LayerNorm(x))): the pre-norm residual pattern of LayerNormResFn with the norm's only consumer, a C -> 4 C Linear (norm2 ->
    mlp.fc1 of a MiT block, mit.py:98,136-146), inside the same formula, so that the backward never writes the Linear's C-wide data gradient
    and reads the hidden-width gradient once: hip.layernorm_linear_bwd forms dy = dh W1, the LayerNorm backward of it and the four
    parameter gradients in one pass.  The forward is one pass too where the library has it for the size (hip.layernorm_linear_fwd: the
    LayerNorm output is neither written nor saved, the backward rebuilds it from x), the two calls LayerNormResFn and LinearFn make
    otherwise; either way h, dx (and the DropPath-scaled copy parked for the producer of x) carry the bits of that pair, the parameter
    gradients are the same sums in another order.  The choice of this formula is made at forward time (layer_norm_res_linear_ok)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, weight, bias, dp_scale=None, dp_rpg=1):
        x, g, b = _ln_enter(ctx, x, gamma, beta, dp_scale, dp_rpg)
        M, K = x.shape
        N = weight.shape[0]
        w = _w(weight.reshape(N, -1), x.dtype)
        if _ln_linear_fwd_fused(x, g, b, w, bias.detach()):
            h, mean, rstd, y, _ = hip.layernorm_linear_fwd(x, g, b, eps, w, bias.detach())
        else:
            y, mean, rstd = hip.layernorm_fwd(x, g, b, eps)
            h = hip.gemm(0, y, w, M, N, K, bias=bias.detach())
        ctx.save_for_backward(x, g, mean, rstd, y, w, b)
        ctx.wshape = weight.shape
        return x.view_as(x), h

    @staticmethod
    def backward(ctx, dres, dh):
        x, g, mean, rstd, y, w, b = ctx.saved_tensors
        if dh is None:
            return dres, None, None, None, None, None, None, None
        dh = dh if dh.is_contiguous() else dh.contiguous()
        if dres is not None and not dres.is_contiguous():
            dres = dres.contiguous()
        dx, dg, db, dw, db1 = _ln_linear_bwd(ctx, dh, dres, x, g, b, mean, rstd, y, w, 4, 5)
        return dx, dg, db, None, dw, db1, None, None


def _ln_linear_trained(x, gamma, beta, weight, bias):
    """The part the LayerNorm + Linear formulas' *_ok rules share: a bf16 training pass on the device, all four parameters present and
    trained."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.ndim == 2 and torch.is_grad_enabled() and x.requires_grad):
        return False
    return bias is not None and weight.ndim == 2 and all(p.requires_grad for p in (gamma, beta, weight, bias))


def layer_norm_res_linear_ok(x, gamma, beta, weight, bias):
    """May (x, Linear(LayerNorm(x))) run as LayerNormResLinearFn?  The library's shape / size / policy rule
    (segf_layernorm_linear_bwd_supported), a training pass, and all four parameters present and trained."""
    return _ln_linear_trained(x, gamma, beta, weight, bias) and hip.layernorm_linear_bwd_supported(x.dtype, x.shape[0], x.shape[1], weight.shape[0])


def layer_norm_res_linear(x, gamma, beta, eps, weight, bias):
    """-> (x, Linear(LayerNorm(x))): use the returned x for the residual connection.  One formula where the fused backward exists for the
    shape (layer_norm_res_linear_ok), layer_norm_res + linear otherwise -- the same forward calls either way."""
    if layer_norm_res_linear_ok(x, gamma, beta, weight, bias):
        return LayerNormResLinearFn.apply(x, gamma, beta, eps, weight, bias, *_dp_of(x))
    x, h = layer_norm_res(x, gamma, beta, eps)
    return x, linear(h, weight, bias)


@direct_grads(1, 2)
class LayerNormResPatchFn(Function):
    """LayerNormResFn for the norm in front of a MiT attention with spatial reduction (mit.py:143, 47): besides (x, norm(x)) it returns
    norm(x) a second time in the patch-major row order of the k = s = sr convolution's im2col matrix, [B Ho Wo, sr sr C] -- written by the same
    kernel (no im2col pass); the backward reads that output's gradient in the same order (no col2im pass) and sums it with the other
    consumer's on load, as LayerNormForkFn does for two consumers in token order."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, lw, ls, dp_scale=None, dp_rpg=1):
        x, g, b = _ln_enter(ctx, x, gamma, beta, dp_scale, dp_rpg, patch=(lw, ls))
        y, mean, rstd, col = hip.layernorm_fwd(x, g, b, eps, patch=ctx.patch)
        ctx.save_for_backward(x, g, mean, rstd)
        return x.view_as(x), y, col

    @staticmethod
    def backward(ctx, dres, dy, dcol):
        x, g, mean, rstd = ctx.saved_tensors
        if dy is None and dcol is None:
            return dres, None, None, None, None, None, None, None
        if dy is None:                       # (only the convolution consumed the norm: its gradient back in token order first)
            raise RuntimeError('layer_norm_res_patch: the token-order output received no gradient')
        dy = dy if dy.is_contiguous() else dy.contiguous()
        if dres is not None and not dres.is_contiguous():
            dres = dres.contiguous()
        if dcol is not None and not dcol.is_contiguous():
            dcol = dcol.contiguous()
        dx, dg, db = _ln_bwd(ctx, x, dy, g, mean, rstd, dy2=dcol, dres=dres, dy2_patch=ctx.patch if dcol is not None else None)
        return dx, dg, db, None, None, None, None, None


@direct_grads(1, 2, 6, 7)
class LayerNormResPatchLinearFn(Function):
    """(x, Linear(LayerNorm(x)), im2col matrix of LayerNorm(x)): LayerNormResPatchFn with the norm's token-order consumer, the attention's
    C -> C q Linear (mit.py:45,143), inside the same formula.  The forward is one pass (hip.layernorm_linear_fwd: the token-order LayerNorm
    output is not written; only its patch-major copy is).  The backward is one pass as well where the library has it for the size
    (hip.layernorm_linear_bwd with N = C: dy = dq Wq is never stored, the patch-major gradient joins it on load, y is rebuilt from x); else
    the forward also keeps y and the backward makes the three launches LinearFn and LayerNormResPatchFn make.  q, col, dx and the
    DropPath-scaled copy carry the bits of that pair of formulas; in the one-pass backward the four parameter gradients are the same sums in
    another order."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, lw, ls, weight, bias, dp_scale=None, dp_rpg=1):
        x, g, b = _ln_enter(ctx, x, gamma, beta, dp_scale, dp_rpg, patch=(lw, ls))
        M, K = x.shape
        N = weight.shape[0]
        w = _w(weight.reshape(N, -1), x.dtype)
        if _ln_linear_fwd_fused(x, g, b, w, bias.detach()):
            ctx.one_pass = bool(hip.layernorm_linear_bwd_ex_supported(x.dtype, M, K, N))
            q, mean, rstd, y, col = hip.layernorm_linear_fwd(x, g, b, eps, w, bias.detach(), patch=ctx.patch, keep_y=not ctx.one_pass)
        else:                                    # (a parameter view the vector loads cannot take: the two launches)
            ctx.one_pass = False
            y, mean, rstd, col = hip.layernorm_fwd(x, g, b, eps, patch=ctx.patch)
            q = hip.gemm(0, y, w, M, N, K, bias=bias.detach())
        ctx.save_for_backward(x, g, mean, rstd, y, w, b)
        ctx.wshape = weight.shape
        return x.view_as(x), q, col

    @staticmethod
    def backward(ctx, dres, dq, dcol):
        x, g, mean, rstd, y, w, b = ctx.saved_tensors
        none = (None,) * 10
        if dq is None and dcol is None:
            return (dres,) + none[1:]
        if dq is None:
            raise RuntimeError('layer_norm_res_patch_linear: the Linear output received no gradient')
        dq = dq if dq.is_contiguous() else dq.contiguous()
        if dres is not None and not dres.is_contiguous():
            dres = dres.contiguous()
        if dcol is not None and not dcol.is_contiguous():
            dcol = dcol.contiguous()
        patch = ctx.patch if dcol is not None else None
        if ctx.one_pass:
            dx, dg, db, dw, dbq = _ln_linear_bwd(ctx, dq, dres, x, g, b, mean, rstd, None, w, 6, 7, dy2=dcol, dy2_patch=patch)
            return dx, dg, db, None, None, None, dw, dbq, None, None
        # the three launches of LinearFn.backward + LayerNormResPatchFn.backward
        M, K = x.shape
        N = w.shape[0]
        dy = hip.gemm(1, dq, w, M, K, N)
        dw, dbq = _linear_param_grads(ctx, dq, y, N, K, M, 6, 7, True, ctx.wshape)
        dx, dg, db = _ln_bwd(ctx, x, dy, g, mean, rstd, dy2=dcol, dres=dres, dy2_patch=patch)
        return dx, dg, db, None, None, None, dw, dbq, None, None


def layer_norm_res_patch_linear_ok(x, gamma, beta, weight, bias):
    """May (x, Linear(LayerNorm(x)), col) run as LayerNormResPatchLinearFn?  The library's rule for the one-pass forward
    (segf_layernorm_linear_fwd_supported), a training pass, and all four parameters present and trained."""
    return _ln_linear_trained(x, gamma, beta, weight, bias) and hip.layernorm_linear_fwd_supported(x.dtype, x.shape[0], x.shape[1], weight.shape[0])


def layer_norm_res_patch_linear(x, gamma, beta, eps, W, sr, weight, bias):
    """-> (x, Linear(LayerNorm(x)), im2col matrix of LayerNorm(x) for a k = s = sr convolution): use the returned x for the residual
    connection.  Only where layer_norm_res_patch_linear_ok; layer_norm_res_patch + linear otherwise."""
    return LayerNormResPatchLinearFn.apply(x, gamma, beta, eps, W.bit_length() - 1, sr.bit_length() - 1, weight, bias, *_dp_of(x))


def patch_layout_ok(W, H, sr):
    """layer_norm_res_patch covers maps whose width and reduction ratio are powers of two (every BASELINE geometry)"""
    return (sr > 1 and (sr & (sr - 1)) == 0 and (W & (W - 1)) == 0 and W >= sr and H % sr == 0
            and not hip.policy('no_ln_patch'))


def layer_norm_res_patch(x, gamma, beta, eps, W, sr):
    """-> (x, LayerNorm(x), im2col matrix of LayerNorm(x) for a k = s = sr convolution [rows / sr^2, sr^2 C])"""
    return LayerNormResPatchFn.apply(x, gamma, beta, eps, W.bit_length() - 1, sr.bit_length() - 1, *_dp_of(x))


@direct_grads(1, 2)
class ConvFromColFn(Function):
    """The k = s = sr convolution of MiT's spatial reduction (mit.py:21,48) on an im2col matrix that already exists
    (layer_norm_res_patch): y = col W^T + b; the data gradient is returned in the matrix's own layout."""

    @staticmethod
    def forward(ctx, col, weight, bias, k):
        col = _rowmajor(col)
        M, K = col.shape
        O, Cin = weight.shape[0], weight.shape[1]
        assert K == k * k * Cin
        wmat = _tap_major(weight, col.dtype, ('patch', col.dtype, K), col.device)
        y = hip.gemm(0, col, wmat, M, O, K, bias=bias.detach() if bias is not None else None)
        ctx.save_for_backward(col, wmat)
        ctx.meta = (M, O, K, k, Cin, bias is not None, weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        col, wmat = ctx.saved_tensors
        M, O, K, k, Cin, has_bias, wshape = ctx.meta
        dy = _rowmajor(dy)
        dw, db = _linear_param_grads(ctx, dy, col, O, K, M, 1, 2, has_bias, wshape, taps=k * k)
        dcol = hip.gemm(1, dy, wmat, M, K, O) if ctx.needs_input_grad[0] else None
        return dcol, dw, db, None


def conv_from_col(col, weight, bias, k):
    return ConvFromColFn.apply(col, weight, bias, k)


@direct_grads(1, 2)
class LayerNormForkFn(Function):
    """LayerNorm whose output has TWO consumers (a MiT / ConvNeXt stage output feeds the decode head and the next stage,
    mit.py:196-216): returns the normalised map twice; the backward kernel sums the two incoming gradients on load."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, dp_scale=None, dp_rpg=1):
        x, g, b = _ln_enter(ctx, x, gamma, beta, dp_scale, dp_rpg)
        y, mean, rstd = hip.layernorm_fwd(x, g, b, eps)
        ctx.save_for_backward(x, g, mean, rstd)
        return y, y.view_as(y)

    @staticmethod
    def backward(ctx, dy1, dy2):
        x, g, mean, rstd = ctx.saved_tensors
        if dy1 is None:
            dy1, dy2 = dy2, None
        dy1 = dy1 if dy1.is_contiguous() else dy1.contiguous()
        if dy2 is not None and not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dx, dg, db = _ln_bwd(ctx, x, dy1, g, mean, rstd, dy2=dy2)
        return dx, dg, db, None, None, None


def layer_norm_fork(x, gamma, beta, eps):
    return LayerNormForkFn.apply(x, gamma, beta, eps, *_dp_of(x))


class ForkFn(Function):
    """x -> n aliases of x for n consumers; the backward adds the n gradients with the library's own add kernel (autograd's
    implicit accumulation would run a framework kernel inside the captured step)."""

    @staticmethod
    def forward(ctx, x, n):
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g for g in gs if g is not None]
        if not gs:
            return None, None
        acc = gs[0]
        for g in gs[1:]:
            acc = hip.add(_rowmajor(acc), _rowmajor(g))
        return acc, None


def fork(x, n=2):
    return ForkFn.apply(x, n)


_RNG_SALT = [0]


def stochastic_scales(owner, keep_probs, row_len, device):
    """fp32 [len(keep_probs), row_len]: per entry 1 / kp with probability kp else 0 (DropPath: one row per draw, row_len = batch;
    Dropout2d: one row of B * C entries).  The generator state {seed, launch counter} lives on the device and is advanced by
    the kernel (segf_bernoulli_scale), so a replayed hipGraph draws fresh numbers; seeded from torch.initial_seed() and the
    order in which the layers first draw.  First call per layer = outside graph capture (the warm-up pass)."""
    key = (str(device), tuple(keep_probs), int(row_len))
    st = getattr(owner, '_segf_rng', None)
    if st is None or st[0] != key:
        _RNG_SALT[0] += 1
        seed = (torch.initial_seed() * 6364136223846793005 + _RNG_SALT[0] * 1442695040888963407) & 0x7FFFFFFFFFFFFFFF
        st = (key, torch.tensor([seed, 0], dtype=torch.int64, device=device),
              torch.tensor(list(keep_probs), dtype=torch.float32, device=device))
        owner._segf_rng = st
    return hip.bernoulli_scale(st[1], st[2], len(keep_probs) * int(row_len), int(row_len)).view(len(keep_probs), int(row_len))


@direct_grads(1, 2)
class ConvPatchFn(Function):
    """Strided conv as im2col + MFMA GEMM: PatchEmbed (mit.py:105,127: k7 s4 p3 / k3 s2 p1), the
    spatial-reduction conv (mit.py:21,48: k = s = sr) and ConvNeXt's stem / downsample convs.
    x is either the fp32 NCHW image (image=True) or NHWC tokens [B*H*W, Cin]."""

    @staticmethod
    def forward(ctx, x, weight, bias, geom, image, dtype):
        B, H, W, Cin, k, stride, pad = geom
        O = weight.shape[0]
        Ho = (H + 2 * pad - k) // stride + 1
        Wo = (W + 2 * pad - k) // stride + 1
        K = k * k * Cin
        ld = (K + 7) // 8 * 8
        # the stem (7 x 7 x 3 = 147 columns, 2 M tokens at cfg2): columns padded to whole 32-steps (160) so that the forward
        # product takes the streaming kernel (rows are its MFMA operand as they lie in memory); the pad columns are zeros on
        # both sides.  The tiled kernel spent 392 us on this [2M x 147] -> 32 product, 75 % of its tile columns empty
        stream_form = (image and dtype == torch.bfloat16 and K % 32 != 0 and (K + 31) // 32 * 32 == 160 and O % 32 == 0
                       and B * Ho * Wo >= 16384)
        if stream_form:
            ld = 160
        x = x if x.is_contiguous() else x.contiguous()
        col = hip.im2col(x, dtype, image, B, H, W, Cin, k, k, stride, pad, Ho, Wo, ld)
        b = bias.detach() if bias is not None else None
        if stream_form:
            wsrc = weight.detach().contiguous()

            def make_wpad():                             # rows of [(ky,kx)][ci] at a row stride of `ld`, the pad columns zero
                t = torch.empty((O, ld), dtype=dtype, device=x.device)
                return t, [('perm', wsrc, t, O, Cin, k * k, Cin, ld), ('zero', t[:, K:])]
            wpad = derived_weight(wsrc, ('patch', dtype, ld), make_wpad)
            wmat = wpad[:, :K]
            y = hip.gemm(0, col, wpad, B * Ho * Wo, O, ld, bias=b)
        else:
            wmat = _tap_major(weight, dtype, ('patch', dtype, K), x.device)
            y = hip.gemm(0, col, wmat, B * Ho * Wo, O, K, bias=b)
        # the im2col matrix itself is kept for the weight gradient (k*k/stride^2 <= 3.1x the conv input, < 1 GB in total
        # for SegFormer-B0 at batch 64 out of 288 GB): rebuilding it in backward costs a second pass over the image
        ctx.save_for_backward(col, wmat)
        ctx.meta = (geom, image, dtype, O, Ho, Wo, K, ld, bias is not None, weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        col, wmat = ctx.saved_tensors
        geom, image, dtype, O, Ho, Wo, K, ld, has_bias, wshape = ctx.meta
        B, H, W, Cin, k, stride, pad = geom
        M = B * Ho * Wo
        dy = _rowmajor(dy)
        dx = None
        dw, db = _linear_param_grads(ctx, dy, col, O, K, M, 1, 2, has_bias, wshape, taps=k * k)
        if ctx.needs_input_grad[0] and not image:
            dcol = hip.gemm(1, dy, wmat, M, K, O)
            dx = hip.col2im(dcol, B, H, W, Cin, k, k, stride, pad, Ho, Wo)
        return dx, dw, db, None, None, None


def conv_patch(x, weight, bias, geom, image=False, dtype=None):
    return ConvPatchFn.apply(x, weight, bias, geom, image, dtype or x.dtype)


class AttentionFn(Function):
    """softmax(Q K^T * scale) V per head (mit.py:52-57).  q: [B*N, C]; kv: [B*Nkv, 2C] = [k | v]."""

    @staticmethod
    def forward(ctx, q, kv, B, N, Nkv, heads):
        q, kv = _rowmajor(q), _rowmajor(kv)
        Cc = q.shape[1]
        hd = Cc // heads
        scale = hd ** -0.5
        o, lse = hip.attention_fwd(q, kv[:, :Cc], kv[:, Cc:], B, heads, N, Nkv, hd, scale)
        ctx.save_for_backward(q, kv, o, lse)
        ctx.meta = (B, N, Nkv, heads, hd, scale, Cc)
        return o

    @staticmethod
    def backward(ctx, do):
        q, kv, o, lse = ctx.saved_tensors
        B, N, Nkv, heads, hd, scale, Cc = ctx.meta
        do = _rowmajor(do)
        dkv = torch.empty_like(kv)
        dq = hip.attention_bwd(q, kv[:, :Cc], kv[:, Cc:], o, do, lse, B, heads, N, Nkv, hd, scale, dkv[:, :Cc], dkv[:, Cc:])
        return dq, dkv, None, None, None, None


def attention(q, kv, B, N, Nkv, heads):
    return AttentionFn.apply(q, kv, B, N, Nkv, heads)


def group_token_index(H, W, G, interval, lda):
    """[groups, G*G] int64: for every (group, slot) of CrossFormer's SDA (lda false: adjacent tokens) or LDA (tokens sampled at
    `interval`) grouping of an H x W map, the flat token index r * W + c, or -1 where the slot is padding (crossformer.py:282-313: the map
    is padded on the right and bottom to a multiple of G, of interval * G in LDA mode).  Groups in the reference's order, groups that
    are all padding included.  Pure Python on the CPU: it pins the map the kernel computes for itself (csrc/attention_group.hip never
    reads it)."""
    I = int(interval) if lda else 1
    div = G * I
    Rh, Rw = -(-H // div), -(-W // div)
    out = torch.full((Rh * Rw * I * I, G * G), -1, dtype=torch.int64)
    for rh in range(Rh):
        for rw in range(Rw):
            for ih in range(I):
                for iw in range(I):
                    g = ((rh * Rw + rw) * I + ih) * I + iw
                    for gi in range(G):
                        r = (rh * G + gi) * I + ih
                        if r >= H:
                            continue
                        for gj in range(G):
                            c = (rw * G + gj) * I + iw
                            if c < W:
                                out[g, gi * G + gj] = r * W + c
    return out


class GroupAttentionFn(Function):
    """CrossFormer's attention core (crossformer.py:121-164 inside the grouping of :282-339): per group of G x G tokens and head,
    softmax(scale q k^T + bias[head] + key mask) v, on the qkv Linear's [B*H*W, 3C] output as it lies; o in token order.  Gradients go to
    qkv and to the [heads, G*G, G*G] bias."""

    @staticmethod
    def forward(ctx, qkv, bias, B, H, W, heads, G, interval, lda):
        qkv = _rowmajor(qkv)
        bias = bias.detach().contiguous()
        scale = 32 ** -0.5
        o, lse = hip.group_attention_fwd(qkv, bias, B, H, W, heads, G, interval, lda, scale)
        ctx.save_for_backward(qkv, bias, lse)
        ctx.meta = (B, H, W, heads, G, interval, lda, scale)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, bias, lse = ctx.saved_tensors
        B, H, W, heads, G, interval, lda, scale = ctx.meta
        dqkv, dbias = hip.group_attention_bwd(qkv, bias, _rowmajor(do), lse, B, H, W, heads, G, interval, lda, scale)
        return dqkv, dbias, None, None, None, None, None, None, None


def group_attention(qkv, bias, B, H, W, heads, G, interval, lda):
    """G: the group side in use (after the reference's small-map rule); head dim 32."""
    return GroupAttentionFn.apply(qkv, bias, B, H, W, heads, G, interval, bool(lda))


# ---- CAS-ViT additive token mixer (casvit.py:68-92, 112-138; csrc/token_mixer.hip) ------------------------------------------------
@direct_grads(1)
class QkvSplit3Fn(Function):
    """q, k, v = chunk3(x W^T) (casvit.py:118,133; no bias) as three CONTIGUOUS [M, C] tensors: the three row blocks of the [3C, C] weight
    are multiplied one by one, because q and k go on into the depthwise 3x3 kernels, which take contiguous rows.  The backward
    gathers the three gradients into the columns of one [M, 3C] buffer with the library's copy kernel (one grouped launch) and runs the two
    products of a 3C-wide Linear on it."""

    @staticmethod
    def forward(ctx, x, weight):
        x = _rowmajor(x)
        M, K = x.shape
        N = weight.shape[0]
        assert N % 3 == 0
        Cq = N // 3
        w = _w(weight.reshape(N, -1), x.dtype)
        outs = tuple(hip.gemm(0, x, w[i * Cq:(i + 1) * Cq], M, Cq, K) for i in range(3))
        ctx.save_for_backward(x, w)
        ctx.meta = (M, N, K, weight.shape)
        return outs

    @staticmethod
    def backward(ctx, dq, dk, dv):
        x, w = ctx.saved_tensors
        M, N, K, wshape = ctx.meta
        Cq = N // 3
        dqkv = torch.empty((M, N), dtype=x.dtype, device=x.device)
        jobs = []
        for i, d in enumerate((dq, dk, dv)):
            sl = dqkv[:, i * Cq:(i + 1) * Cq]
            jobs.append(('cast', _rowmajor(d), sl) if d is not None else ('zero', sl))
        hip.prep_grouped(jobs)
        dx = hip.gemm(1, dqkv, w, M, K, N) if ctx.needs_input_grad[0] else None
        dw, _ = _linear_param_grads(ctx, dqkv, x, N, K, M, 1, None, False, wshape)
        return dx, dw


def qkv_split3(x, weight):
    return QkvSplit3Fn.apply(x, weight)


@direct_grads(2)
class SpatialGateFn(Function):
    """(x * s, sum over each sample's pixels of x * s) with s = sigmoid(conv1x1_to_one_channel(r)), r = ReLU(BN(dw3x3(x) + b)):
    SpatialOperation's tail and ChannelOperation's pooled sum (casvit.py:75-80, 86).  Kernel: spatial_gate_fwd_kernel / _bwd_kernel."""

    @staticmethod
    def forward(ctx, x, r, weight, B, HW):
        r = r if r.is_contiguous() else r.contiguous()
        x = _rowmajor(x)
        w = weight.detach().reshape(-1).contiguous()
        y, s, pool = hip.spatial_gate_fwd(x, r, w, B, HW)
        ctx.save_for_backward(x, r, s, w)
        ctx.meta = (B, HW, weight.shape)
        return y, pool

    @staticmethod
    def backward(ctx, dy, dpool):
        x, r, s, w = ctx.saved_tensors
        B, HW, wshape = ctx.meta
        if dy is None:
            dy = hip.zeros((B * HW, w.numel()), x.dtype, x.device)
        if dpool is not None:
            dpool = dpool.detach().float().contiguous()
        dx, dr, dw = hip.spatial_gate_bwd(_rowmajor(dy), dpool, x, r, s, w, B, HW)
        return dx, dr, dw.view(wshape), None, None


def spatial_gate(x, r, weight, B, HW):
    return SpatialGateFn.apply(x, r, weight, B, HW)


class ChannelGateMixFn(Function):
    """u = q1 * gq[b] + k1 * gk[b]: the two ChannelOperation products and the q + k of casvit.py:92,136 in one pass; gq, gk fp32 [B, C].
    Kernel: channel_gate_mix_fwd_kernel / _bwd_kernel."""

    @staticmethod
    def forward(ctx, q1, k1, gq, gk, B, HW):
        q1, k1 = _rowmajor(q1), _rowmajor(k1)
        gq, gk = gq.detach().float().contiguous(), gk.detach().float().contiguous()
        u = hip.channel_gate_mix_fwd(q1, k1, gq, gk, B, HW)
        ctx.save_for_backward(q1, k1, gq, gk)
        ctx.meta = (B, HW)
        return u

    @staticmethod
    def backward(ctx, du):
        q1, k1, gq, gk = ctx.saved_tensors
        B, HW = ctx.meta
        dq1, dk1, dgq, dgk = hip.channel_gate_mix_bwd(_rowmajor(du), q1, k1, gq, gk, B, HW)
        return dq1, dk1, dgq, dgk, None, None


def channel_gate_mix(q1, k1, gq, gk, B, HW):
    return ChannelGateMixFn.apply(q1, k1, gq, gk, B, HW)


class GatedMulFn(Function):
    """z = a * v (casvit.py:136: dwc(q + k) * v).  Kernel: gated_mul_fwd_kernel / _bwd_kernel."""

    @staticmethod
    def forward(ctx, a, v):
        a, v = _rowmajor(a), _rowmajor(v)
        ctx.save_for_backward(a, v)
        return hip.gated_mul_fwd(a, v)

    @staticmethod
    def backward(ctx, dz):
        a, v = ctx.saved_tensors
        return hip.gated_mul_bwd(_rowmajor(dz), a, v)


def gated_mul(a, v):
    return GatedMulFn.apply(a, v)


# ---- MetaFormer / ConvFormer (metaformer.py:198-241, 489-513; csrc/metaformer.hip) ----------------------------------------------------
@direct_grads(1, 2)
class StarReLUFn(Function):
    """s * relu(u)^2 + b with one-element learnable s and b (metaformer.py:224-241).  The kernels read s and b from device memory (no
    host read: the call can be captured) and the backward writes the two whole-tensor sums into the parameters' flat-gradient views.
    Kernel: starrelu_fwd_kernel / starrelu_bwd_kernel + starrelu_finalize_kernel."""

    @staticmethod
    def forward(ctx, u, scale, bias):
        u = _rowmajor(u)
        s, b = scale.detach().reshape(1), bias.detach().reshape(1)
        ctx.save_for_backward(u, s)
        ctx.pshapes = (scale.shape, bias.shape)
        return hip.starrelu_fwd(u, s, b)

    @staticmethod
    def backward(ctx, dy):
        u, s = ctx.saved_tensors
        gs, gb = gslot(ctx, 1), gslot(ctx, 2)
        du, ds, db = hip.starrelu_bwd(u, _rowmajor(dy), s, ds=gs.view(1) if gs is not None else None, db=gb.view(1) if gb is not None else None)
        return du, ds.view(ctx.pshapes[0]), db.view(ctx.pshapes[1])


def star_relu(u, scale, bias):
    return StarReLUFn.apply(u, scale, bias)


@direct_grads(1)
class ColScaleFn(Function):
    """x * scale[c] (Scale on the skip path of stages 3 and 4, metaformer.py:198-208, 501, 507).  Kernel: colscale_fwd_kernel /
    colscale_bwd_kernel + colreduce_finalize."""

    @staticmethod
    def forward(ctx, x, scale):
        x = _rowmajor(x)
        sc = scale.detach().reshape(-1).contiguous()
        ctx.save_for_backward(x, sc)
        ctx.pshape = scale.shape
        return hip.colscale_fwd(x, sc)

    @staticmethod
    def backward(ctx, dy):
        x, sc = ctx.saved_tensors
        gs = gslot(ctx, 1)
        dx, dscale = hip.colscale_bwd(_rowmajor(dy), x, sc, dscale=gs.view(-1) if gs is not None and gs.is_contiguous() else None)
        return dx, dscale.view(ctx.pshape)


def col_scale(x, scale):
    return ColScaleFn.apply(x, scale)


@direct_grads(1, 2)
class DWConvGeluFn(Function):
    """gelu(depthwise3x3(x) + b) on NHWC tokens (mit.py:62-71 + F.gelu at :99)."""

    @staticmethod
    def forward(ctx, x, weight, bias, B, H, W, apply_gelu):
        x = x if x.is_contiguous() else x.contiguous()
        Cc = x.shape[1]
        w9 = weight.detach().reshape(Cc, 9).contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        y = hip.dwconv3x3_gelu_fwd(x, w9, b, B, H, W, Cc, apply_gelu)
        ctx.save_for_backward(x, w9, b)
        ctx.meta = (B, H, W, Cc, apply_gelu, weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w9, b = ctx.saved_tensors
        B, H, W, Cc, apply_gelu, wshape = ctx.meta
        dy = dy if dy.is_contiguous() else dy.contiguous()
        gw, gb = gslot(ctx, 1), (gslot(ctx, 2) if b is not None else None)       # flat-gradient views: written in place, no copy
        if _FIN_QUEUE is not None and _adjacent_slots(ctx, 1, 2) is not None:
            # the finalize of the (dw, db) partial sums joins the step's grouped finalize launches (one instead of two launches per block)
            dx, item = hip.dwconv3x3_gelu_bwd(x, w9, b, dy, B, H, W, Cc, apply_gelu, dw_out=gw, db_out=gb, defer=True)
            _queue_finalizes(ctx, (item, (1, 2)))
            return dx, None, None, None, None, None, None
        dx, dw, db = hip.dwconv3x3_gelu_bwd(x, w9, b, dy, B, H, W, Cc, apply_gelu, dw_out=gw, db_out=gb)
        return dx, dw.view(wshape), (db if b is not None else None), None, None, None, None


def dwconv3x3_gelu(x, weight, bias, B, H, W, apply_gelu=True):
    return DWConvGeluFn.apply(x, weight, bias, B, H, W, apply_gelu)


@direct_grads(1, 2, 3, 4)
class DWConvGeluLinearFn(Function):
    """y = residual + rscale[b] * (gelu(depthwise3x3(x) + b9) W2^T + b2): the tail of MiT's Mix-FFN (mit.py:98-99) as ONE formula, so that
    its backward never writes the hidden-width gradient of fc2's input: hip.dwconv3x3_gelu_bwd_fc2 rebuilds those values from the
    C-wide output gradient inside the depthwise backward's first pass.  The forward makes the two calls DWConvGeluFn and LinearFn make;
    every gradient has the bits of that pair.  The choice of this formula is made at forward time (dwconv3x3_gelu_linear_ok) and the entry point
    checks the walk form again when the backward runs: a dispatch switch (SEGFAC_DW_NO_WALK, ..._DW_NO_SMALL) flipped between the two makes the
    backward raise (SEGF_ERR_SHAPE) rather than take another path.  Argument order: fc2's parameters at 1, 2 (the slots _queue_dw reads), the depthwise
    ones at 3, 4."""

    @staticmethod
    def forward(ctx, x, weight2, bias2, weight, bias, B, H, W, residual, rscale):
        x = x if x.is_contiguous() else x.contiguous()
        M, Cc = x.shape
        N = weight2.shape[0]
        w9 = weight.detach().reshape(Cc, 9).contiguous()
        b = bias.detach().contiguous()
        g = hip.dwconv3x3_gelu_fwd(x, w9, b, B, H, W, Cc, True)
        w2 = _w(weight2.reshape(N, -1), x.dtype)
        y = hip.gemm(0, g, w2, M, N, Cc, bias=bias2.detach(), residual=residual, rscale=rscale, rows_per_group=H * W)
        ctx.save_for_backward(x, w9, b, g, w2, rscale)
        ctx.meta = (B, H, W, Cc, N, M, weight.shape, weight2.shape, residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w9, b, g, w2, rscale = ctx.saved_tensors
        B, H, W, Cc, N, M, wshape, w2shape, has_res = ctx.meta
        dy = _rowmajor(dy)
        dys = _scaled_dy(dy, rscale, H * W) if rscale is not None else dy
        dw2, db2 = _linear_param_grads(ctx, dys, g, N, Cc, M, 1, 2, True, w2shape)
        gw, gb = gslot(ctx, 3), gslot(ctx, 4)
        dres = dy if (has_res and ctx.needs_input_grad[8]) else None
        if _FIN_QUEUE is not None and _adjacent_slots(ctx, 3, 4) is not None:
            dx, item = hip.dwconv3x3_gelu_bwd_fc2(x, w9, b, dys, w2, B, H, W, Cc, N, dw_out=gw, db_out=gb, defer=True)
            _queue_finalizes(ctx, (item, (3, 4)))
            return dx, dw2, db2, None, None, None, None, None, dres, None
        dx, dw, db = hip.dwconv3x3_gelu_bwd_fc2(x, w9, b, dys, w2, B, H, W, Cc, N, dw_out=gw, db_out=gb)
        return dx, dw2, db2, dw.view(wshape), db, None, None, None, dres, None


def dwconv3x3_gelu_linear_ok(x, weight2, bias2, weight, bias, B, H, W):
    """May gelu(dwconv3x3(x)) -> Linear run as DWConvGeluLinearFn?  The library's shape / size / policy rule
    (segf_dwconv3x3_gelu_bwd_fc2_supported), a training pass, and all four parameters present and trained."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and torch.is_grad_enabled() and x.requires_grad):
        return False
    if bias is None or bias2 is None or not all(p.requires_grad for p in (weight2, bias2, weight, bias)):
        return False
    return (hip.dwconv3x3_gelu_bwd_fc2_supported(x.dtype, B, H, W, x.shape[1], weight2.shape[0])
            or hip.dwconv3x3_gelu_bwd_fc2_lds_supported(x.dtype, B, H, W, x.shape[1], weight2.shape[0]))


def dwconv3x3_gelu_linear(x, weight2, bias2, weight, bias, B, H, W, residual=None, rscale=None):
    y = DWConvGeluLinearFn.apply(x, weight2, bias2, weight, bias, B, H, W, residual, rscale)
    if rscale is not None:
        y._segf_dp = (rscale, H * W)                            # as functional.linear tags its residual form
    return y


def _bn_mean_rstd(x, training, pre_sums, running_mean, running_var, momentum, eps):
    """(mean, rstd) fp32 [C] of a BatchNorm over the rows of x.  Training: batch statistics -- from pre_sums, fp32 [2, C] (sum, sum of
    squares) per channel, where x's producer already summed them, else from a pass over x -- and the running buffers are updated in
    place; evaluation: the running buffers as they stand."""
    if training and pre_sums is not None:
        return hip.bn_stats_from_sums(pre_sums, x.shape[0], running_mean, running_var, momentum, eps)
    if training:
        return hip.bn_stats(x, running_mean, running_var, momentum, eps)
    return running_mean.detach().clone(), torch.rsqrt(running_var.detach() + eps)


@direct_grads(1, 2)
class BatchNormActFn(Function):
    """BatchNorm2d (+ReLU/ReLU6) (+Dropout2d channel scale) on NHWC rows.
    ConvModule of heads/segformer.py:21-29, layers/conv_module.py:4-9, mobilenetv2.py:5-11; Dropout2d of
    heads/segformer.py:40,57.  Training uses batch statistics and updates the running buffers in place."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, act, chan_scale, rows_per_sample,
                pre_sums=None):
        x = x if x.is_contiguous() else x.contiguous()
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        mean, rstd = _bn_mean_rstd(x, training, pre_sums, running_mean, running_var, momentum, eps)
        y = hip.bn_apply(x, mean, rstd, g, b, act, chan_scale, rows_per_sample or 1)
        ctx.save_for_backward(x, mean, rstd, g, b, chan_scale)
        ctx.meta = (act, rows_per_sample or 1, not training)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, g, b, chan_scale = ctx.saved_tensors
        act, rps, eval_mode = ctx.meta
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dx, dg, db = hip.bn_bwd(x, dy, mean, rstd, g, b, act, chan_scale, rps, eval_mode)
        return dx, dg, db, None, None, None, None, None, None, None, None, None


def batch_norm_act(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, act=1, chan_scale=None,
                   rows_per_sample=None, pre_sums=None):
    return BatchNormActFn.apply(x, gamma, beta, running_mean, running_var, training, momentum, eps, act, chan_scale,
                                rows_per_sample, pre_sums)


@direct_grads(1, 2, 11, 12)
class BnActLinearFn(Function):
    """ConvModule's BatchNorm2d + ReLU, the Dropout2d channel scale and the following 1x1 conv (heads/segformer.py:21-29,40,
    57-58: linear_fuse.bn/activate -> dropout -> linear_pred) as ONE product: the normalisation is folded into per-(sample,
    channel) scale / shift tables and applied while the GEMM stages its activation operand, in the forward product and again in
    the weight-gradient product, so the normalised [B*H*W, E] tensor is never written.  Same arithmetic as
    BatchNormActFn + LinearFn (bf16 rounding of the normalised value included)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, act, chan_scale, rps, weight, bias, Np,
                pre_sums, fold_slot=None):
        ctx.fold_slot = fold_slot
        x = x if x.is_contiguous() else x.contiguous()
        M, K = x.shape
        N = weight.shape[0]
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        mean, rstd = _bn_mean_rstd(x, training, pre_sums, running_mean, running_var, momentum, eps)
        scale, shift = hip.bn_affine_table(mean, rstd, g, b, chan_scale, M // rps, K)
        w, bp = _padded_rows(weight, bias, N, Np, K, x.dtype, x.device)
        y = hip.gemm_pro(0, x, w, M, Np, K, scale, shift, rps, act, bias=bp)[:, :N]
        ctx.save_for_backward(x, mean, rstd, g, b, chan_scale, scale, shift, w)
        ctx.meta = (M, N, K, Np, act, rps, not training, bias is not None, weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, g, b, chan_scale, scale, shift, w = ctx.saved_tensors
        M, N, K, Np, act, rps, eval_mode, has_bias, wshape = ctx.meta
        if dy.stride(-1) == 1 and dy.stride(0) == Np:
            dyp = dy.as_strided((M, Np), (Np, 1))           # the producer zero-fills the pad columns (segfac.h)
        else:
            dyp = hip.zeros((M, Np), x.dtype, x.device)
            hip.cast2d(_rowmajor(dy), dyp[:, :N])
        # the bias gradient rides on pass 1 of the fused BatchNorm backward where that form carries the weight gradient too
        # (segf_bn_cls_bwd_full_db): no column-sum pass of its own over the class gradients
        ride_db = (has_bias and act in (0, 1) and not hip.policy('no_head_fused_cw')
                   and hip.bn_cls_bwd_full_db_supported(x.dtype, M, K, Np, rps))
        db = hip.colsum(dyp)[:N] if has_bias and not ride_db else None
        dw = None
        if hip.bn_cls_bwd_supported(x.dtype, M, K, Np, rps):
            # da = dyp W is recomputed inside both BatchNorm passes (K = #classes terms per element) instead of being written
            # once and read twice: 19.8 -> 10.9 GB at cfg2, batch 128 (head_fused.hip)
            slot = ctx.fold_slot
            x1 = slot.get('x1') if slot is not None else None
            ride_dg = x1 is not None and x1.shape[0] == M and hip.bn_cls_bwd_dw_supported(x.dtype, M, K, Np, rps, x1.shape[1])
            if act in (0, 1) and not hip.policy('no_head_fused_cw'):
                # ... and the classifier's own weight gradient rides on the first pass (it has the x and dy tiles on chip), as the
                # stage-1 weight gradient of the folded head rides on the second: no separate pass over x for either
                if ride_db:
                    dx, dg, dbeta, dG, dwc, dbc = hip.bn_cls_bwd_full_db(dyp, w, x, mean, rstd, g, b, act, chan_scale, rps, eval_mode,
                                                                         x1=x1 if ride_dg else None)
                    db = dbc[:N]
                else:
                    dx, dg, dbeta, dG, dwc = hip.bn_cls_bwd_full(dyp, w, x, mean, rstd, g, b, act, chan_scale, rps, eval_mode,
                                                                 x1=x1 if ride_dg else None)
                dw = dwc[:N].view(wshape)
                if ride_dg:
                    slot['dG'] = dG
            elif ride_dg:
                # x is the folded SegFormerHead's stride-4 map: the weight-gradient product of its stage-1 term (dx^T x1 and the
                # column sums of dx) rides on the second BatchNorm pass, which has the dx tile on chip (one 3.2 GB pass less)
                dx, dg, dbeta, slot['dG'] = hip.bn_cls_bwd_dw(dyp, w, x, mean, rstd, g, b, act, chan_scale, rps, eval_mode, x1)
            else:
                dx, dg, dbeta = hip.bn_cls_bwd(dyp, w, x, mean, rstd, g, b, act, chan_scale, rps, eval_mode)
        else:
            da = hip.gemm(1, dyp, w, M, K, Np)               # gradient w.r.t. the (never materialised) normalised tensor
            dx, dg, dbeta = hip.bn_bwd(x, da, mean, rstd, g, b, act, chan_scale, rps, eval_mode)
        if dw is None:
            dw = hip.gemm_pro(2, dyp, x, Np, K, M, scale, shift, rps, act, split_k=_splitk(Np, K, M))[:N].view(wshape)
        return dx, dg, dbeta, None, None, None, None, None, None, None, None, dw, db, None, None, None


def bn_act_linear(x, gamma, beta, running_mean, running_var, training, momentum, eps, act, chan_scale, rows_per_sample, weight,
                  bias, pad_to=None, pre_sums=None):
    """batch_norm_act followed by linear; fused into the GEMM operand load when the shape takes the 256-tile kernel.
    pre_sums: optional fp32 [2, C] (sum, sum of squares) of x per channel from its producer (replaces the statistics pass)."""
    M, K = x.shape
    N = weight.shape[0]
    Np = pad_to if (pad_to and pad_to > N) else N
    rps = rows_per_sample or M
    if (x.dtype == torch.bfloat16 and act in (0, 1) and M % rps == 0 and hip.gemm_pro_supported(x.dtype, 0, M, Np, K, rps)
            and hip.gemm_pro_supported(x.dtype, 2, Np, K, M, rps)):
        return BnActLinearFn.apply(x, gamma, beta, running_mean, running_var, training, momentum, eps, act, chan_scale, rps,
                                   weight, bias, Np, pre_sums, getattr(x, '_segf_fold', None))
    y = batch_norm_act(x, gamma, beta, running_mean, running_var, training, momentum, eps, act, chan_scale, rows_per_sample,
                       pre_sums=pre_sums)
    return linear(y, weight, bias, pad_to=pad_to)


@direct_grads(5, 6, 7, 8, 9, 10, 11, 12)
class SegformerProjectConcatFn(Function):
    """The front half of SegFormerHead.forward (heads/segformer.py:42-50): per-scale Linear(C_i -> E),
    bilinear resize to the stride-4 grid, channel concat in the order [c4, c3, c2, c1].  Every branch writes
    straight into its column slice of one [B*H1*W1, 4E] buffer -- no torch.cat copy."""

    @staticmethod
    def forward(ctx, geoms, *args):
        feats, weights, biases = args[0:4], args[4:8], args[8:12]
        B = geoms[0][0]
        H1, W1 = geoms[0][1], geoms[0][2]
        E = weights[0].shape[0]
        dtype = feats[0].dtype
        M1 = B * H1 * W1
        cat = torch.empty((M1, 4 * E), dtype=dtype, device=feats[0].device)
        saved = []
        for i in range(4):
            f = _rowmajor(feats[i])
            w = _w(weights[i], dtype)
            _, h, wd = geoms[i]
            sl = cat[:, (3 - i) * E:(4 - i) * E]
            if i == 0:
                hip.gemm(0, f, w, M1, E, f.shape[1], out=sl, bias=biases[i].detach())
            else:
                t = hip.gemm(0, f, w, B * h * wd, E, f.shape[1], bias=biases[i].detach())
                hip.bilinear_fwd(t, B, h, wd, E, H1, W1, sl, align_corners=False)
            saved += [f, w]
        ctx.save_for_backward(*saved)
        ctx.meta = (geoms, E)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        geoms, E = ctx.meta
        saved = ctx.saved_tensors
        dcat = _rowmajor(dcat)
        B, H1, W1 = geoms[0]
        dfs, dws, dbs = [], [], []
        for i in range(4):
            f, w = saved[2 * i], saved[2 * i + 1]
            _, h, wd = geoms[i]
            sl = dcat[:, (3 - i) * E:(4 - i) * E]
            dy = sl if i == 0 else hip.bilinear_bwd(sl, B, h, wd, E, H1, W1, align_corners=False)
            M, Ci = f.shape
            dfs.append(hip.gemm(1, dy, w, M, Ci, E) if ctx.needs_input_grad[1 + i] else None)
            dws.append(hip.gemm(2, dy, f, E, Ci, M, out_dtype=torch.float32, split_k=_splitk(E, Ci, M)))
            dbs.append(hip.colsum(dy))
        return (None, *dfs, *dws, *dbs)


def segformer_project_concat(feats, weights, biases, geoms):
    return SegformerProjectConcatFn.apply(tuple(geoms), *feats, *weights, *biases)


@direct_grads(5, 6, 7, 8, 9, 10, 11, 12, 13)
class SegformerFoldedFuseFn(Function):
    """linear_fuse.conv( cat_i( resize( linear_c{i}(x_i) ) ) ) of SegFormerHead.forward (heads/segformer.py:42-56) with
    the algebra folded: Linear -> bilinear resize -> concat -> 1x1 conv (no bias) is affine in x_i, and bilinear resizing
    commutes with affine maps (its weights sum to one), so
        y = sum_i resize_i( x_i G_i^T ) + beta,   G_i = F_i W_i  [E, C_i],   beta = sum_i F_i b_i,
    where F_i is the column block of the fuse weight that multiplies scale i in the reversed concat [c4, c3, c2, c1].
    The [B*H1*W1, 4E] concat buffer and the 4E -> E GEMM over it (77 of the model's 89 GFLOP/img at cfg2) never exist;
    the per-scale products run at native resolution (1.6 GFLOP/img).  The backward returns gradients for the ORIGINAL
    parameters (linear_c{i}.proj.{weight,bias}, linear_fuse.conv.weight) by the chain rule through G_i and beta."""

    @staticmethod
    def forward(ctx, geoms, *args):
        feats, weights, biases, wf = args[0:4], args[4:8], args[8:12], args[12]
        ctx.fold_slot = args[13] if len(args) > 13 else None
        B, H1, W1 = geoms[0]
        E = weights[0].shape[0]
        dtype = feats[0].dtype
        dev = feats[0].device
        wf32 = wf.detach().reshape(E, 4 * E)
        wfc = _w(wf32 if wf32.is_contiguous() else wf32.contiguous(), dtype)
        ts, saved = [], []
        # one launch for the whole stride-4 map (x1 G1^T and the three resizes as one accumulated matrix product per 8 x 8 pixel
        # block, csrc/fuse_map.hip) when the geometry is the 1/2-1/4-1/8 pyramid; the stage-1 bias then rides in the 1/2 map
        one_pass = (dtype == torch.bfloat16 and all(geoms[i] == (B, H1 >> i, W1 >> i) for i in (1, 2, 3))
                    and hip.fuse_map_248_supported(dtype, B, H1, W1, E, feats[0].shape[1]))
        G1, beta1 = None, None
        # W'_i = [W_i | b_i | 0] (bias as one extra input column): one GEMM yields G_i = F_i W_i and beta_i = F_i b_i.  The packing of
        # the four W'_i is ONE launch, the unpacking of the four products another (hip.prep_grouped) -- at batch 4 these 24 jobs were
        # 24 launches of the launch floor each
        xs, Wps, Gps, Gs, betas, jobs = [], [], [], [], [], []
        for i in range(4):
            x = _rowmajor(feats[i])
            Ci = x.shape[1]
            Wp = torch.empty((E, Ci + 8), dtype=dtype, device=dev)
            jobs += [('cast', weights[i].detach(), Wp[:, :Ci]), ('cast', biases[i].detach().unsqueeze(1), Wp[:, Ci:Ci + 1]),
                     ('zero', Wp[:, Ci + 1:])]
            xs.append(x)
            Wps.append(Wp)
        hip.prep_grouped(jobs)
        jobs = []
        for i in range(4):
            Ci = xs[i].shape[1]
            Fi = wfc[:, (3 - i) * E:(4 - i) * E]
            Gp = hip.gemm(1, Fi, Wps[i], E, Ci + 8, E, out_dtype=torch.float32)                # [E, Ci+8] fp32
            G = torch.empty((E, Ci), dtype=dtype, device=dev)
            beta_i = torch.empty(E, dtype=torch.float32, device=dev)
            jobs += [('cast', Gp[:, :Ci], G), ('cast', Gp[:, Ci:Ci + 1], beta_i.unsqueeze(1))]
            Gps.append(Gp)
            Gs.append(G)
            betas.append(beta_i)
        hip.prep_grouped(jobs)
        for i in range(4):
            x, G, beta_i, Wp = xs[i], Gs[i], betas[i], Wps[i]
            Ci = x.shape[1]
            _, h, w = geoms[i]
            if one_pass and i == 0:
                G1, beta1 = G, beta_i
                ts.append(None)
            else:
                if one_pass and i == 1:
                    beta_i = hip.add(beta_i.unsqueeze(0), beta1.unsqueeze(0)).squeeze(0)    # a constant passes through the resize
                ts.append(hip.gemm(0, x, G, B * h * w, E, Ci, bias=beta_i))   # a constant row passes through the resize unchanged
            saved += [x, G, Wp]
            if i == 0 and ctx.fold_slot is not None and dtype == torch.bfloat16:
                ctx.fold_slot['x1'] = x           # BnActLinearFn.backward may compute dG_1 while it has the gradient tile on chip
        if one_pass:
            y, sums = hip.fuse_map_248(saved[0], G1, ts[1], ts[2], ts[3], B, H1, W1)
        else:
            y, sums = hip.upsample_add_stats(ts[0], [(ts[i], geoms[i][1], geoms[i][2]) for i in range(1, 4)], B, H1, W1, E)
        if sums is None:
            sums = torch.empty(0, device=y.device)          # geometry without the fused statistics: the consumer runs its own pass
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(wfc, *saved)
        ctx.meta = (geoms, E, dtype)
        return y, sums

    @staticmethod
    def backward(ctx, dy, _dsums=None):
        geoms, E, dtype = ctx.meta
        sv = ctx.saved_tensors
        wfc = sv[0]
        B, H1, W1 = geoms[0]
        dy = _rowmajor(dy)
        dev = dy.device
        dbeta = None                         # [E] fp32 = colsum(dy) (colsum(resize^T(dy)) == colsum(dy): the resize weights sum
                                             # to one); it rides along with the stage-1 weight-gradient product below
        dwf = torch.empty((E, 4 * E), dtype=torch.float32, device=dev)
        dxs, dws, dbs = [], [], []
        dts = None
        if (H1 % 8 == 0 and W1 % 8 == 0 and E % 8 == 0 and not hip.policy('no_bwd248')
                and all(geoms[i][1:] == (H1 >> i, W1 >> i) for i in (1, 2, 3))):
            dts = hip.bilinear_bwd_248(dy, B, H1, W1, E)          # the three transposed resizes in ONE pass over dy
        dGps = []
        for i in range(4):
            x, G, Wp = sv[1 + 3 * i], sv[2 + 3 * i], sv[3 + 3 * i]
            _, h, w = geoms[i]
            M, Ci = x.shape
            dt = dy if i == 0 else (dts[i - 1] if dts is not None else hip.bilinear_bwd(dy, B, h, w, E, H1, W1, align_corners=False))
            dxs.append(hip.gemm(1, dt, G, M, Ci, E) if ctx.needs_input_grad[1 + i] else None)
            pre = ctx.fold_slot.pop('dG', None) if (i == 0 and ctx.fold_slot is not None) else None
            if pre is not None and tuple(pre.shape) == (E, Ci + 8):
                dGp = pre                          # [dy^T x_1 | colsum(dy) | 0] arrived with dy (segf_bn_cls_bwd_dw)
                dbeta = dGp[:, Ci]
            else:
                dGp = torch.empty((E, Ci + 8), dtype=torch.float32, device=dev)             # d [G_i | . ]: the product fills [:, :Ci]
                if i == 0:
                    _, dbeta = hip.gemm_dw_db(dt, x, E, Ci, M, split_k=_splitk(E, Ci, M), out=dGp[:, :Ci])
                else:
                    hip.gemm(2, dt, x, E, Ci, M, out=dGp[:, :Ci], split_k=_splitk(E, Ci, M))
            dGps.append(dGp)
        # d [G_i | beta_i | 0] in the compute dtype, all four in one launch
        dGcs, jobs = [], []
        for i in range(4):
            Ci = sv[1 + 3 * i].shape[1]
            if dtype == torch.float32:
                dGc = dGps[i]
                jobs += [('zero', dGc[:, Ci + 1:])] + ([('cast', dbeta.unsqueeze(1), dGc[:, Ci:Ci + 1])] if dbeta.data_ptr() != dGc[:, Ci].data_ptr() else [])
            else:
                dGc = torch.empty((E, Ci + 8), dtype=dtype, device=dev)
                jobs += [('cast', dGps[i][:, :Ci], dGc[:, :Ci]), ('cast', dbeta.unsqueeze(1), dGc[:, Ci:Ci + 1]), ('zero', dGc[:, Ci + 1:])]
            dGcs.append(dGc)
        hip.prep_grouped(jobs)
        for i in range(4):
            Wp, dGc = sv[3 + 3 * i], dGcs[i]
            Ci = sv[1 + 3 * i].shape[1]
            Fi = wfc[:, (3 - i) * E:(4 - i) * E]
            hip.gemm(0, dGc, Wp, E, E, Ci + 8, out=dwf[:, (3 - i) * E:(4 - i) * E])          # dF_i = dG_i W_i^T + dbeta b_i^T
            dWp = hip.gemm(2, Fi, dGc, E, Ci + 8, E, out_dtype=torch.float32)               # [dW_i | db_i | 0] = F_i^T dG'_i
            dws.append(dWp[:, :Ci])
            dbs.append(dWp[:, Ci])
        if ctx.fold_slot is not None:
            ctx.fold_slot.clear()
        return (None, *dxs, *dws, *dbs, dwf.view(E, 4 * E, 1, 1), None)


def segformer_folded_fuse(feats, weights, biases, fuse_weight, geoms):
    """-> (y [B*H1*W1, E], sums): sums = fp32 [2, E] per-channel (sum, sum of squares) of y for the BatchNorm that follows, or
    None when the geometry did not take the fused kernel."""
    slot = {}
    y, sums = SegformerFoldedFuseFn.apply(tuple(geoms), *feats, *weights, *biases, fuse_weight, slot)
    y._segf_fold = slot          # read by bn_act_linear: its backward can compute this function's stage-1 weight gradient in passing
    return y, (sums if sums.numel() else None)


@direct_grads(1, 2)
class DWConv7Fn(Function):
    """Depthwise 7x7 conv + bias on NHWC tokens (ConvNeXt Block.dwconv, convnext.py:29,39; convnextv2.py:88,101)."""

    @staticmethod
    def forward(ctx, x, weight, bias, B, H, W):
        x = x if x.is_contiguous() else x.contiguous()
        Cc = x.shape[1]
        wsrc = weight.detach().contiguous()

        def make_wt():
            t = torch.empty((49, Cc), dtype=torch.float32, device=x.device)
            return t, [('perm', wsrc, t, 1, Cc, 49, Cc)]
        wt = derived_weight(wsrc, ('dw7',), make_wt)                                              # [49][C] fp32
        y = hip.dwconv7x7_fwd(x, wt, bias.detach() if bias is not None else None, B, H, W, Cc)
        ctx.save_for_backward(x, wt)
        ctx.meta = (B, H, W, Cc, weight.shape, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wt = ctx.saved_tensors
        B, H, W, Cc, wshape, has_bias = ctx.meta
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dx, dw, db = hip.dwconv7x7_bwd(x, wt, dy, B, H, W, Cc, need_dx=ctx.needs_input_grad[0], need_db=has_bias)
        return dx, dw.view(wshape), db, None, None, None


def dwconv7x7(x, weight, bias, B, H, W):
    return DWConv7Fn.apply(x, weight, bias, B, H, W)


@direct_grads(1)
class Conv3x3Fn(Function):
    """3x3 / stride 1 / pad 1 convolution without bias on NHWC tokens as an implicit MFMA GEMM (ConvModule(c1, c2, 3, 1, 1):
    heads/upernet.py:26,28, modules/ppm.py:19, heads/fpn.py:19).  x may be a column slice of a wider concat buffer."""

    @staticmethod
    def forward(ctx, x, weight, B, H, W, fp8=False):
        x = _rowmajor(x)
        O, I = weight.shape[0], weight.shape[1]
        wm = _tap_major(weight, x.dtype, ('conv3x3', x.dtype), x.device)
        use8 = bool(fp8) and x.dtype == torch.bfloat16 and hip.conv3x3_fp8_supported(0, B, H, W, I, O)
        xq = sx = None
        if use8:
            # fp8 forward (BASELINE cfg5): activations e4m3 with one dynamic scale for the tensor, weights e4m3 per output channel
            xq, sx = hip.quant_tensor_fp8(x)
            wq, sw = hip.quant_rows_fp8(wm)
            y = hip.conv3x3_fp8(0, xq, sx, wq, sw, B, H, W, I, O)
        else:
            y = hip.conv3x3(0, x, wm, B, H, W, I, O)
        # the quantised input is kept for the fp8 weight gradient (one byte per element next to the bf16 tensor autograd keeps anyway)
        keep8 = use8 and hip.conv3x3_fp8_wgrad_supported(B, H, W, I, O)
        ctx.save_for_backward(x, weight.detach(), xq if keep8 else None, sx if keep8 else None)
        ctx.meta = (B, H, W, I, O, weight.shape, bool(fp8))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, xq, sx = ctx.saved_tensors
        B, H, W, I, O, wshape, fp8 = ctx.meta
        dy = _rowmajor(dy)
        dx = dw = None
        gq = sg = None
        if fp8 and dy.dtype == torch.bfloat16 and (xq is not None or (ctx.needs_input_grad[0] and hip.conv3x3_fp8_supported(1, B, H, W, I, O))):
            gq, sg = hip.quant_tensor_fp8(dy, e5m2=True)          # the gradient in e5m2, one dynamic scale: data and weight gradient share it
        if ctx.needs_input_grad[0]:
            wt = _tap_major_transposed(w, dy.dtype)
            if gq is not None and hip.conv3x3_fp8_supported(1, B, H, W, I, O):
                wq, sw = hip.quant_rows_fp8(wt)                   # transposed weights e4m3 per input channel
                dx = hip.conv3x3_fp8(1, gq, sg, wq, sw, B, H, W, I, O)
            else:
                dx = hip.conv3x3(1, dy, wt, B, H, W, I, O)
        if ctx.needs_input_grad[1]:
            if gq is not None and xq is not None:
                dwm = hip.conv3x3_fp8_wgrad(xq, sx, gq, sg, B, H, W, I, O)
            else:
                dwm = hip.conv3x3(2, x, dy, B, H, W, I, O, split_k=hip.pick_splitk_conv3x3(I, O, B * H * W))           # [O][(ky,kx)][ci] fp32
            dw = _from_tap_major(dwm, O, 9, I).view(wshape)
        return dx, dw, None, None, None, None


def conv3x3(x, weight, B, H, W, fp8=False):
    """bf16: implicit GEMM (fp8=True: forward and data gradient on fp8 operands where the shape takes the 256-tile kernel); fp32
    parity mode: im2col + exact-fp32 GEMM (ConvPatchFn)."""
    if x.dtype == torch.bfloat16 and weight.shape[0] % 8 == 0 and weight.shape[1] % 8 == 0:
        return Conv3x3Fn.apply(x, weight, B, H, W, fp8)
    return ConvPatchFn.apply(x, weight, None, (B, H, W, weight.shape[1], 3, 1, 1), False, x.dtype)


@direct_grads(1)
class DilatedConv3x3Fn(Function):
    """3x3 / stride 1 / padding = dilation convolution without bias on NHWC tokens as an implicit MFMA GEMM over the taps that can touch
    the map (_ASPPConv, heads/deeplabv3.py:65-75), bf16 or fp32.  x may be a column slice of a wider buffer."""

    @staticmethod
    def forward(ctx, x, weight, B, H, W, dilation):
        x = _rowmajor(x)
        O, I = weight.shape[0], weight.shape[1]
        wm = _tap_major(weight, x.dtype, ('conv3x3', x.dtype), x.device)
        y = hip.conv3x3_dil(0, x, wm, B, H, W, I, O, dilation)
        ctx.save_for_backward(x, weight.detach())
        ctx.meta = (B, H, W, I, O, weight.shape, dilation)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        B, H, W, I, O, wshape, dilation = ctx.meta
        dy = _rowmajor(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wt = _tap_major_transposed(w, dy.dtype)
            dx = hip.conv3x3_dil(1, dy, wt, B, H, W, I, O, dilation)
        if ctx.needs_input_grad[1]:
            dwm = hip.conv3x3_dil(2, x, dy, B, H, W, I, O, dilation)                                        # [O][(ky,kx)][ci] fp32
            dw = _from_tap_major(dwm, O, 9, I).view(wshape)
        return dx, dw, None, None, None, None


def conv3x3_dilated(x, weight, B, H, W, dilation):
    """Conv2d(c1, c2, 3, padding=dilation, dilation=dilation, bias=False).  dilation 1 is the plain 3x3 convolution (conv3x3)."""
    dilation = int(dilation)
    if dilation == 1:
        return conv3x3(x, weight, B, H, W)
    O, I = weight.shape[0], weight.shape[1]
    if not hip.conv3x3_dil_supported(x.dtype, 0, B, H, W, I, O, dilation):
        raise ValueError(f'conv3x3_dilated: no kernel for {x.dtype} B={B} H={H} W={W} {I}->{O} dilation={dilation} '
                         '(channels must be multiples of 8, dilation >= 1)')
    return DilatedConv3x3Fn.apply(x, weight, B, H, W, dilation)


class DropoutFn(Function):
    """nn.Dropout per element (heads/deeplabv3.py:56,115): y = x * scale with scale = keep / p_keep; the backward multiplies by the
    same scales."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.save_for_backward(scale)
        return hip.mul_scale(_rowmajor(x), scale)

    @staticmethod
    def backward(ctx, dy):
        scale, = ctx.saved_tensors
        return hip.mul_scale(_rowmajor(dy), scale), None


def dropout(x, p, training, owner, override=None):
    """Elementwise dropout with rate p on token rows.  Eval mode and p == 0 apply nothing.  override: a 0 / 1 keep mask of x's shape
    (tests); otherwise the keep-scales come from the device-side generator (stochastic_scales), fresh on every graph replay."""
    if not training or p <= 0.0:
        return x
    keep = 1.0 - float(p)
    if override is not None:
        scale = (override.to(device=x.device, dtype=torch.float32) / keep).reshape(x.shape).contiguous()
    else:
        scale = stochastic_scales(owner, (keep,), x.shape[0] * x.shape[1], x.device).view(x.shape)
    return DropoutFn.apply(x, scale)


class GeluFn(Function):
    """nn.GELU (erf) between ConvNeXt's pointwise linears (convnext.py:32,43)."""

    @staticmethod
    def forward(ctx, u):
        u = u if u.is_contiguous() else u.contiguous()
        ctx.save_for_backward(u)
        return hip.gelu_fwd(u)

    @staticmethod
    def backward(ctx, dy):
        (u,) = ctx.saved_tensors
        return hip.gelu_bwd(u, dy if dy.is_contiguous() else dy.contiguous())


def gelu(u):
    return GeluFn.apply(u)


@direct_grads(1, 2, 3)
class LinearLayerScaleFn(Function):
    """x_in + drop_path( gamma * (x W^T + b) )  (convnext.py:44-49).  The layer scale is folded into the parameters
    (W' = diag(gamma) W, b' = gamma o b) so the activation is never touched; gradients for W, b and gamma follow by the
    chain rule: dW = gamma o dW', db = gamma o db', dgamma[c] = <dW'[c], W[c]> + db'[c] b[c]."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, residual, rscale, rows_per_group):
        x = _rowmajor(x)
        M, K = x.shape
        N = weight.shape[0]
        w32, b32, g32 = weight.detach(), bias.detach(), gamma.detach().contiguous()
        ws = hip.scale_rows(w32 if w32.is_contiguous() else w32.contiguous(), g32, 1)              # fp32 [N, K]
        bs = hip.scale_rows(b32.view(N, 1), g32, 1).view(N)
        wc = _w(ws, x.dtype)
        y = hip.gemm(0, x, wc, M, N, K, bias=bs, residual=residual, rscale=rscale, rows_per_group=rows_per_group or 1)
        ctx.save_for_backward(x, wc, w32, b32, g32, rscale)
        ctx.meta = (M, N, K, residual is not None, rows_per_group or 1)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wc, w32, b32, g32, rscale = ctx.saved_tensors
        M, N, K, has_res, rpg = ctx.meta
        dy = _rowmajor(dy)
        dys = hip.scale_rows(dy, rscale, rpg) if rscale is not None else dy
        dx = hip.gemm(1, dys, wc, M, K, N) if ctx.needs_input_grad[0] else None
        dws, dbs = hip.gemm_dw_db(dys, x, N, K, M, split_k=_splitk(N, K, M))                         # d W', d b'
        dw = hip.scale_rows(dws, g32, 1)
        db = hip.scale_rows(dbs.view(N, 1), g32, 1).view(N)
        dg = hip.rowdot(dws, w32 if w32.is_contiguous() else w32.contiguous(), dbs, b32)
        return dx, dw, db, dg, (dy if has_res else None), None, None


def linear_layer_scale(x, weight, bias, gamma, residual=None, rscale=None, rows_per_group=None):
    return LinearLayerScaleFn.apply(x, weight, bias, gamma, residual, rscale, rows_per_group)


@direct_grads(1, 2)
class GRNFn(Function):
    """Global Response Normalization of ConvNeXtV2 (convnextv2.py:68-80) on NHWC tokens; gamma / beta are [1,1,1,C].
    pre_gelu: GRN(gelu(x)) with the activation applied inside the GRN kernels (convnextv2.py:92-94: act then grn) -- gelu(x) is
    never materialised and the backward returns the gradient of the pre-activation."""

    @staticmethod
    def forward(ctx, x, gamma, beta, B, rows_per_sample, pre_gelu=False):
        x = x if x.is_contiguous() else x.contiguous()
        g = gamma.detach().reshape(-1).contiguous()
        b = beta.detach().reshape(-1).contiguous()
        y, sq = hip.grn_fwd(x, g, b, B, rows_per_sample, pre_gelu)
        ctx.save_for_backward(x, g, sq)
        ctx.meta = (B, rows_per_sample, gamma.shape, bool(pre_gelu))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, sq = ctx.saved_tensors
        B, rps, pshape, pre_gelu = ctx.meta
        dx, dg, db = hip.grn_bwd(x, dy if dy.is_contiguous() else dy.contiguous(), g, sq, B, rps, pre_gelu)
        return dx, dg.view(pshape), db.view(pshape), None, None, None


def grn(x, gamma, beta, B, rows_per_sample, pre_gelu=False):
    return GRNFn.apply(x, gamma, beta, B, rows_per_sample, pre_gelu)


class AdaptiveAvgPoolFn(Function):
    """nn.AdaptiveAvgPool2d(S) on NHWC tokens (modules/ppm.py:13)."""

    @staticmethod
    def forward(ctx, x, B, H, W, S):
        x = x if x.is_contiguous() else x.contiguous()
        ctx.meta = (B, H, W, x.shape[1], S)
        return hip.adaptive_avgpool(x, B, H, W, x.shape[1], S)

    @staticmethod
    def backward(ctx, dy):
        B, H, W, Cc, S = ctx.meta
        return hip.adaptive_avgpool(dy if dy.is_contiguous() else dy.contiguous(), B, H, W, Cc, S, bwd=True), None, None, None, None


def adaptive_avgpool(x, B, H, W, S):
    return AdaptiveAvgPoolFn.apply(x, B, H, W, S)


class UpsampleAddFn(Function):
    """lateral + F.interpolate(top, size=lateral.shape[-2:], bilinear, align_corners=False)  (heads/upernet.py:41)."""

    @staticmethod
    def forward(ctx, base, top, geom):
        B, H, W, h, w = geom
        base, top = _rowmajor(base), _rowmajor(top)
        ctx.meta = (geom, base.shape[1])
        return hip.upsample_add(base, [(top, h, w)], B, H, W, base.shape[1])

    @staticmethod
    def backward(ctx, dy):
        (B, H, W, h, w), Cc = ctx.meta
        dy = _rowmajor(dy)
        dtop = hip.bilinear_bwd(dy, B, h, w, Cc, H, W, align_corners=False) if ctx.needs_input_grad[1] else None
        return dy, dtop, None


def upsample_add(base, top, geom):
    return UpsampleAddFn.apply(base, top, tuple(geom))


class ResizeConcatFn(Function):
    """torch.cat([F.interpolate(f_i, size=(H, W), bilinear, align_corners=ac_i) ...], dim=1) on NHWC tokens: every branch is
    written straight into its column slice of one [B*H*W, sum C_i] buffer (modules/ppm.py:23-26, heads/upernet.py:45-49).
    A branch that already has the target size is copied (F.interpolate to the same size is the identity)."""

    @staticmethod
    def forward(ctx, geoms, aligns, size, *feats):
        B, H, W = size
        Cs = [f.shape[1] for f in feats]
        cat = torch.empty((B * H * W, sum(Cs)), dtype=feats[0].dtype, device=feats[0].device)
        off = 0
        for f, (h, w), ac, Cc in zip(feats, geoms, aligns, Cs):
            f = _rowmajor(f)
            sl = cat[:, off:off + Cc]
            if (h, w) == (H, W):
                hip.cast2d(f, sl)
            else:
                hip.bilinear_fwd(f, B, h, w, Cc, H, W, sl, align_corners=ac)
            off += Cc
        ctx.meta = (geoms, aligns, size, Cs)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        geoms, aligns, (B, H, W), Cs = ctx.meta
        dcat = _rowmajor(dcat)
        grads, off = [], 0
        for i, ((h, w), ac, Cc) in enumerate(zip(geoms, aligns, Cs)):
            sl = dcat[:, off:off + Cc]
            if not ctx.needs_input_grad[3 + i]:
                grads.append(None)
            elif (h, w) == (H, W):
                grads.append(sl)
            else:
                grads.append(hip.bilinear_bwd(sl, B, h, w, Cc, H, W, align_corners=ac))
            off += Cc
        return (None, None, None, *grads)


def resize_concat(feats, geoms, aligns, size):
    return ResizeConcatFn.apply(tuple(geoms), tuple(aligns), tuple(size), *feats)


class AddFn(Function):
    """x + y on token rows (the residual of mobilenetv2.InvertedResidual, mobilenetv2.py:33-35)."""

    @staticmethod
    def forward(ctx, a, b):
        return hip.add(_rowmajor(a), _rowmajor(b))

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    return AddFn.apply(a, b)


class SubsampleFn(Function):
    """x[:, ::s, ::s, :] on NHWC tokens, rows (oy, ox) <- (s*oy, s*ox): a stride-s convolution with padding 1 and kernel 3 equals
    the stride-1 convolution sampled at every s-th position, which is how MobileNetV2's four stride-2 depthwise layers
    (mobilenetv2.py:27, ConvModule(ch, ch, 3, s, 1, g=ch)) run on the stride-1 depthwise kernel.  Forward = im2col with a 1x1
    window, backward = its col2im."""

    @staticmethod
    def forward(ctx, x, B, H, W, stride):
        x = x if x.is_contiguous() else x.contiguous()
        Cc = x.shape[1]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        ctx.meta = (B, H, W, Cc, stride, Ho, Wo)
        return hip.im2col(x, x.dtype, False, B, H, W, Cc, 1, 1, stride, 0, Ho, Wo, Cc)

    @staticmethod
    def backward(ctx, dy):
        B, H, W, Cc, stride, Ho, Wo = ctx.meta
        dy = dy if dy.is_contiguous() else dy.contiguous()
        return hip.col2im(dy, B, H, W, Cc, 1, 1, stride, 0, Ho, Wo), None, None, None, None


def subsample(x, B, H, W, stride):
    return SubsampleFn.apply(x, B, H, W, stride)


class NearestUpFn(Function):
    """F.interpolate(x, mode='nearest') by integer factors (+ base): heads/fpn.py:31 (`size=`), :34-35 (`out + lateral`, then
    `scale_factor=2.0`)."""

    @staticmethod
    def forward(ctx, x, base, geom):
        B, h, w, H, W = geom
        x = x if x.is_contiguous() else x.contiguous()
        if base is not None:
            base = base if base.is_contiguous() else base.contiguous()
        ctx.meta = (geom, x.shape[1], base is not None)
        return hip.nearest_up(x, B, h, w, x.shape[1], H, W, base=base)

    @staticmethod
    def backward(ctx, dy):
        (B, h, w, H, W), Cc, has_base = ctx.meta
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dx = hip.nearest_up(dy, B, h, w, Cc, H, W, bwd=True) if ctx.needs_input_grad[0] else None
        return dx, (dy if has_base else None), None


def nearest_up(x, geom, base=None):
    """geom = (B, h, w, H, W)."""
    return NearestUpFn.apply(x, base, tuple(geom))


class UpsampleCEDiceFn(Function):
    """criterion(F.interpolate(logits, size), target): build_models.py:65 + engine.py:10-15 +
    util/losses.py:126-177, without materialising full-resolution logits in the forward."""

    @staticmethod
    def forward(ctx, logits, target, geom, ignore_index, class_weight, dice):
        B, Cc, h, w, H, W = geom
        logits = _rowmajor(logits)
        # the kernel reads `target` as int64 [B, H, W] on the device: anything else would be silently reinterpreted
        # (F.cross_entropy raises for non-Long targets, engine.py:12)
        if not target.is_cuda or target.device != logits.device:
            raise RuntimeError('criterion: target must be a device tensor on the logits\' device (no CPU fallback)')
        if target.dtype != torch.int64:
            raise RuntimeError(f'criterion: expected an int64 (Long) target, got {target.dtype}')
        if target.numel() != B * H * W:
            raise RuntimeError(f'criterion: target has {target.numel()} elements, expected B*H*W = {B * H * W}')
        if logits.shape[0] != B * h * w or logits.shape[1] < Cc:
            raise RuntimeError(f'criterion: logits {tuple(logits.shape)} do not match geometry {geom}')
        target = target.contiguous()
        # lse: the per-pixel log-sums the forward leaves for the backward (None where the configuration has no such path)
        # (grad mode is always off inside Function.forward and _rowmajor may have copied: the autograd context knows whether a backward
        # can follow)
        loss, stats, lse = hip.ce_dice_fwd(logits, B, Cc, h, w, H, W, target, ignore_index, class_weight, dice,
                                           want_lse=bool(ctx.needs_input_grad[0]))
        ctx.save_for_backward(logits, target, stats, class_weight, lse)
        ctx.meta = (geom, ignore_index, dice)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)          # (no zero-fill launches for the gradients of the two auxiliary outputs)
        return loss[0], loss.detach(), stats

    @staticmethod
    def backward(ctx, gloss, _gparts, _gstats):
        logits, target, stats, cw, lse = ctx.saved_tensors
        (B, Cc, h, w, H, W), ignore_index, dice = ctx.meta
        if gloss is None:                           # only the detached parts were used downstream
            return None, None, None, None, None, None
        go = gloss.reshape(1).to(torch.float32).contiguous()
        dl = hip.ce_dice_bwd(logits, B, Cc, h, w, H, W, target, ignore_index, cw, dice, stats, go, lse=lse)[:, :Cc]
        return dl, None, None, None, None, None


def upsample_ce_dice(logits, target, geom, ignore_index=255, class_weight=None, dice=True):
    """Returns (loss, parts[3] = {total, ce, dice_loss}, stats)."""
    return UpsampleCEDiceFn.apply(logits, target, tuple(geom), int(ignore_index), class_weight, bool(dice))


class UpsamplePixelLossFn(Function):
    """OhemCrossEntropy / FocalLoss of util/losses.py:9-66 on F.interpolate(logits, size) (build_models.py:65) without the
    full-resolution logits: the forward leaves the fp32 per-pixel CE map and the device-side selection state, the backward
    reads both (include/segfac.h, segf_pixel_loss_*)."""

    @staticmethod
    def forward(ctx, logits, target, geom, mode, params, ignore_index, class_weight):
        B, Cc, h, w, H, W = geom
        logits = _rowmajor(logits)
        if not target.is_cuda or target.device != logits.device:
            raise RuntimeError('pixel loss: target must be a device tensor on the logits\' device (no CPU fallback)')
        if target.dtype != torch.int64:
            raise RuntimeError(f'pixel loss: expected an int64 (Long) target, got {target.dtype}')
        if target.numel() != B * H * W:
            raise RuntimeError(f'pixel loss: target has {target.numel()} elements, expected B*H*W = {B * H * W}')
        if logits.shape[0] != B * h * w or logits.shape[1] < Cc:
            raise RuntimeError(f'pixel loss: logits {tuple(logits.shape)} do not match geometry {geom}')
        if not hip.pixel_loss_supported(logits.dtype, mode, B, Cc, h, w, H, W):
            raise RuntimeError(f'pixel loss: geometry {geom} / {logits.dtype} has no kernel (C <= 192, B*H*W < 2^31)')
        target = target.contiguous()
        p0, p1, size_average = params
        loss, ce_map, state = hip.pixel_loss_fwd(logits, B, Cc, h, w, H, W, target, ignore_index, class_weight, mode, p0, p1,
                                                 size_average)
        ctx.save_for_backward(logits, target, class_weight, ce_map, state)
        ctx.meta = (geom, mode, params, ignore_index)
        info = state[:8]
        ctx.mark_non_differentiable(ce_map, info)
        ctx.set_materialize_grads(False)
        return loss[0], ce_map, info

    @staticmethod
    def backward(ctx, gloss, _gmap, _ginfo):
        logits, target, cw, ce_map, state = ctx.saved_tensors
        (B, Cc, h, w, H, W), mode, (p0, p1, size_average), ignore_index = ctx.meta
        if gloss is None:
            return None, None, None, None, None, None, None
        go = gloss.reshape(1).to(torch.float32).contiguous()
        dl = hip.pixel_loss_bwd(logits, B, Cc, h, w, H, W, target, ignore_index, cw, mode, p0, p1, size_average, ce_map, state,
                                go)[:, :Cc]
        return dl, None, None, None, None, None, None


PIXEL_INFO_FIELDS = ('n_valid', 'n_min', 'n_hard', 'n_gt', 'n_eq', 'used_topk', 'kappa', 'bad_label')


def upsample_pixel_loss(logits, target, geom, mode, params, ignore_index=255, class_weight=None):
    """mode 'ohem', params (theta,): OhemCrossEntropy with theta = float32(-log(thresh)); mode 'focal', params (alpha, gamma,
    size_average): FocalLoss.  Returns (loss, ce_map [B, H, W] fp32, info); info is the int32[8] head of the device state in the
    order of PIXEL_INFO_FIELDS (kappa: fp32 bits, see pixel_loss_info).  ce_map and info are non-differentiable."""
    if mode == 'ohem':
        code, prm = hip.PIXEL_OHEM, (float(params[0]), 0.0, 1)
    elif mode == 'focal':
        code, prm = hip.PIXEL_FOCAL, (float(params[0]), float(params[1]), 1 if params[2] else 0)
    else:
        raise ValueError(f"upsample_pixel_loss: mode must be 'ohem' or 'focal', got {mode!r}")
    return UpsamplePixelLossFn.apply(logits, target, tuple(geom), code, prm, int(ignore_index), class_weight)


def pixel_loss_info(info):
    """Host dict of upsample_pixel_loss's info (one synchronising copy): the integers plus kappa as a Python float."""
    host = info.detach().cpu()
    out = dict(zip(PIXEL_INFO_FIELDS, host.tolist()))
    out['kappa'] = host[6:7].view(torch.float32).item()
    return out


class UpsampleToNCHWFn(Function):
    """F.interpolate(head_out, size=input, bilinear, align_corners=False) -> fp32 NCHW logits
    (build_models.py:65), for callers that want the reference's materialised tensor."""

    @staticmethod
    def forward(ctx, logits, geom):
        B, Cc, h, w, H, W = geom
        logits = _rowmajor(logits)
        ctx.meta = (geom, logits.dtype, logits.stride(0))
        return hip.bilinear_to_nchw_f32(logits, B, h, w, Cc, H, W)

    @staticmethod
    def backward(ctx, dout):
        (B, Cc, h, w, H, W), dtype, ld = ctx.meta
        dn = hip.permute021(dout.contiguous(), B, Cc, H * W, dtype).view(B * H * W, Cc)   # NCHW -> NHWC
        dl = hip.bilinear_bwd(dn, B, h, w, Cc, H, W, align_corners=False, ld_in=ld)[:, :Cc]
        return dl, None


def upsample_to_nchw(logits, geom):
    return UpsampleToNCHWFn.apply(logits, tuple(geom))


class NCHWToTokensFn(Function):
    """[B, C, H, W] -> token rows [B*H*W, C] through the re-layout kernel (both directions)."""

    @staticmethod
    def forward(ctx, x):
        B, Cc, H, W = x.shape
        ctx.meta = (B, Cc, H, W, x.dtype)
        return hip.permute021(x.contiguous(), B, Cc, H * W, x.dtype).view(B * H * W, Cc)

    @staticmethod
    def backward(ctx, dt):
        B, Cc, H, W, dtype = ctx.meta
        return hip.permute021(_rowmajor(dt).contiguous(), B, H * W, Cc, dtype).view(B, Cc, H, W)


def nchw_to_tokens(x):
    return NCHWToTokensFn.apply(x)
