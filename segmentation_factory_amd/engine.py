"""criterion / train_one_epoch / evaluate with the reference's signatures (engine.py:10-104).

Differences that are deliberate: compute is bf16-with-fp32-accumulate inside
the kernels instead of fp16 autocast + GradScaler; when the model offers ``forward_lowres`` the loss and the
eval metrics consume the stride-4 head output directly (fused upsample), so the 157 MB/img full-resolution
logits tensor is never written.
"""
import math
import sys

import torch

from . import functional as Fh
from . import hip
from . import utils
from .backbones import TokenMap, tokens_from_nchw
from .metrics import Metrics


def _class_weight(loss_weight, device):
    if loss_weight is None:
        return None
    return torch.as_tensor(loss_weight, dtype=torch.float32, device=device).contiguous()


def criterion_lowres(lowres: TokenMap, target, size, loss_weight=None, num_classes: int = 2, dice: bool = True,
                     ignore_index: int = -100):
    """criterion(F.interpolate(head_out, size), target) without materialising the upsampled logits."""
    H, W = size
    nc = lowres.data.shape[1]
    assert nc == num_classes, (nc, num_classes)
    loss, parts, _ = Fh.upsample_ce_dice(lowres.data, target, (lowres.B, nc, lowres.H, lowres.W, H, W), ignore_index,
                                         _class_weight(loss_weight, target.device), dice is True)
    return loss


def criterion(inputs, target, loss_weight=None, num_classes: int = 2, dice: bool = True, ignore_index: int = -100):
    """engine.py:10-15: F.cross_entropy + (dice) util.losses.dice_loss on [B, C, H, W] logits."""
    if isinstance(inputs, TokenMap):
        return criterion_lowres(inputs, target, target.shape[-2:], loss_weight, num_classes, dice, ignore_index)
    B, C, H, W = inputs.shape
    dtype = inputs.dtype if inputs.dtype in (torch.float32, torch.bfloat16) else torch.float32
    t = inputs.permute(0, 2, 3, 1)
    if t.is_contiguous() and inputs.dtype == dtype:
        tm = TokenMap(t.reshape(B * H * W, C), B, H, W)              # zero-copy: already NHWC underneath
    else:
        tm = TokenMap(Fh.nchw_to_tokens(inputs.to(dtype)), B, H, W)
    return criterion_lowres(tm, target, (H, W), loss_weight, num_classes, dice, ignore_index)


class _DeferredLosses:
    """Device ring of the last steps' loss values (graph path of train_one_epoch): `push` is one 4-byte device copy behind the
    replayed step, `drain` is the one host synchronisation of a logging interval."""

    def __init__(self, device, capacity):
        self.ring = torch.zeros(capacity, 1, dtype=torch.float32, device=device)
        self.meta, self.n = [], 0

    def full(self):
        return self.n == self.ring.shape[0]

    def push(self, loss, lr, it):
        hip.cast2d(loss.detach().reshape(1, 1), self.ring[self.n:self.n + 1])
        self.meta.append((lr, it))
        self.n += 1

    def drain(self):
        vals = self.ring[:self.n, 0].cpu().tolist()          # the synchronisation point
        out = [(v, lr, it) for v, (lr, it) in zip(vals, self.meta)]
        self.meta, self.n = [], 0
        return out


def _flush_losses(pending, metric_logger, writer, print_freq, it0):
    for loss_value, lr, it in pending.drain():
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping training".format(loss_value))
            sys.exit(1)
        metric_logger.update(loss=loss_value, lr=lr)
        if writer is not None and (it - it0) % print_freq == 0:
            writer.add_scalar('train_loss', loss_value, it)
            writer.add_scalar('train_lr', lr, it)


def _graph_step_wanted(args, model, core, optimizer, loss_scaler, device):
    """The step runs as a replayed hipGraph (graph.GraphedTrainStep) unless the caller opted out.  `args.hip_graph`: True = required
    (a capture failure raises), False = eager launches, absent / None = AUTO: what `python train_gpu.py ...` as the reference's
    README launches it gets (train_gpu.py:325) -- the graph whenever the pieces it drives are the product's own (a model with
    `forward_lowres`, one of the fused flat-buffer optimizers, the no-scaling NativeScaler) and the model is not already wrapped in
    DistributedDataParallel (whose hooks then carry the exchange); an earlier failed capture on this model keeps it eager."""
    from .optim import FusedFlatOptimizer, NativeScaler
    pref = getattr(args, 'hip_graph', None)
    if pref is not None and not pref:
        return False
    ok = (hasattr(core, 'forward_lowres') and isinstance(optimizer, FusedFlatOptimizer) and torch.device(device).type == 'cuda')
    if pref:
        return ok
    return (ok and isinstance(loss_scaler, NativeScaler) and not hasattr(model, 'module')
            and getattr(core, '_graph_disabled', None) is None)


def _fall_back_to_eager(core, model, optimizer, device, err):
    """AUTO mode only: the capture of the train step failed (a plugin module that synchronises or allocates on another stream, tied
    weights, out of memory during the warm-up passes ...).  Say why, undo what the attempt armed, and continue with per-kernel
    launches in THIS process -- never a re-exec.  Under several ranks the graph path would have carried the gradient exchange: a
    DistributedDataParallel wrapper (the reference's own, train_gpu.py:233-236) takes it over."""
    print(f'[segmentation_factory_amd] hipGraph capture of the train step failed ({type(err).__name__}: {str(err)[:300]}); '
          'continuing with eager launches (pass --no-hip-graph to skip the attempt)', flush=True)
    core._graph_disabled = f'{type(err).__name__}: {err}'
    core._graphed_step = None
    if hasattr(optimizer, 'disable_direct_grads'):
        optimizer.disable_direct_grads()
    for p in core.parameters():
        p.grad = None
    torch.cuda.synchronize()
    if utils.get_world_size() > 1 and not hasattr(model, 'module'):
        dev = torch.device(device)
        core._ddp_fallback = torch.nn.parallel.DistributedDataParallel(
            core, device_ids=[dev.index if dev.index is not None else torch.cuda.current_device()], find_unused_parameters=True)
        return core._ddp_fallback
    return model


def _named_loss(args):
    """The loss class `args.loss` names (losses.py; util/losses.py of the reference), or None for the engine's own criterion
    (`loss` absent, None or 'ce_dice').  Two-class runs get the weights engine.py:28-32 gives its criterion; FocalLoss takes none."""
    name = getattr(args, 'loss', None)
    if name is None or name == 'ce_dice':
        return None
    from . import losses
    weight = [1.0, 2.0] if args.nb_classes == 2 else None
    if name == 'CrossEntropy':
        return losses.CrossEntropy(args.ignore_index, weight)
    if name == 'OhemCrossEntropy':
        return losses.OhemCrossEntropy(args.ignore_index, weight, thresh=getattr(args, 'ohem_thresh', 0.7))
    if name == 'FocalLoss':
        return losses.FocalLoss(getattr(args, 'focal_alpha', 1.0), getattr(args, 'focal_gamma', 0.0), True, args.ignore_index)
    raise ValueError(f"args.loss: expected ce_dice, CrossEntropy, OhemCrossEntropy or FocalLoss, got {name!r}")


def train_one_epoch(model, optimizer, dataloader, epoch, device, print_freq, clip_grad, clip_mode, loss_scaler,
                    writer=None, args=None):
    model.train()
    num_steps = len(dataloader)
    metric_logger = utils.MetricLogger(delimiter="  ")
    metric_logger.add_meter('lr', utils.SmoothedValue(window_size=1, fmt='{value:.6f}'))
    header = 'Epoch: [{}]'.format(epoch)
    loss_weight = torch.as_tensor([1.0, 2.0], device=device) if args.nb_classes == 2 else None   # engine.py:28-32
    core = model.module if hasattr(model, 'module') else model
    fused = hasattr(core, 'forward_lowres')
    # built once per model and configuration: the captured step of a later epoch keeps calling the object it was captured with
    loss_key = tuple(getattr(args, k, None) for k in ('loss', 'ohem_thresh', 'focal_alpha', 'focal_gamma', 'nb_classes', 'ignore_index'))
    if getattr(core, '_named_loss', (None, None))[0] != loss_key:
        core._named_loss = (loss_key, _named_loss(args))
    named_loss = core._named_loss[1]
    use_graph = _graph_step_wanted(args, model, core, optimizer, loss_scaler, device)
    if getattr(core, '_ddp_fallback', None) is not None:
        model = core._ddp_fallback      # an earlier capture failed under several ranks: DistributedDataParallel carries the exchange

    pending = None
    for idx, (img, lbl) in enumerate(metric_logger.log_every(dataloader, print_freq, header)):
        img = img.to(device, non_blocking=True)
        lbl = lbl.to(device, non_blocking=True)
        if use_graph:
            # the whole step (zero_grad, forward, criterion, backward, gradient gather) replayed as one hipGraph, followed by
            # the RCCL all-reduce of the flat gradient buffer and the fused AGC/AdamW kernel (graph.py)
            from .graph import GraphedTrainStep
            key = (tuple(img.shape), tuple(lbl.shape), clip_grad, clip_mode) + ((loss_key,) if named_loss is not None else ())
            gs = getattr(core, '_graphed_step', None)
            if gs is None or gs.key != key:
                def loss_fn(m, x, y, _lw=loss_weight, _hw=tuple(img.shape[2:])):
                    if named_loss is not None:
                        return named_loss(m.forward_lowres(x), y)
                    return criterion_lowres(m.forward_lowres(x), y, _hw, _lw, num_classes=args.nb_classes, dice=args.dice,
                                            ignore_index=args.ignore_index)
                core._graphed_step = gs = None
                try:
                    gs = GraphedTrainStep(core, optimizer, loss_fn, (img, lbl), clip_grad=clip_grad, clip_mode=clip_mode,
                                          exchange=getattr(args, 'grad_exchange', None), payload=getattr(args, 'grad_payload', None))
                except Exception as e:      # noqa: BLE001 -- whatever stopped the capture, the eager launches below still train
                    if getattr(args, 'hip_graph', None):
                        raise               # asked for explicitly (--hip-graph): the failure is the caller's to see
                    model = _fall_back_to_eager(core, model, optimizer, device, e)
                    use_graph = False
                if gs is not None:
                    gs.key = key
                    core._graphed_step = gs
                    print(f'[segmentation_factory_amd] train step captured as one hipGraph (input {tuple(img.shape)}, '
                          f'{"bucketed gradient exchange over " + str(gs.world) + " ranks" if gs.exchanging else "single rank"})', flush=True)
        if use_graph:
            if getattr(dataloader, 'bind_output', None) is not None and getattr(dataloader, 'out', None) is None:
                dataloader.bind_output(gs.static_inputs)    # device-side input pipeline: later batches land in the step's buffers
            loss = gs.step(img, lbl)
            lr = optimizer.param_groups[0]["lr"]
            # ONE host synchronisation per logging interval instead of one per step (the reference reads
            # loss.item() and calls torch.cuda.synchronize() every step, engine.py:44,56): the step's loss is parked in a device
            # ring, and the meters / the non-finite check / the TensorBoard scalars see every value, in order, when the line is due
            if pending is None:
                pending = _DeferredLosses(loss.device, max(1, min(int(print_freq), 256)))
            pending.push(loss, lr, epoch * num_steps + idx)
            if idx % print_freq == 0 or idx == num_steps - 1 or pending.full():
                _flush_losses(pending, metric_logger, writer if getattr(args, 'local_rank', 0) == 0 else None, print_freq, epoch * num_steps)
            continue
        optimizer.zero_grad()
        if fused:
            # DDP hooks fire on backward through the wrapped module's parameters either way
            if hasattr(model, 'module'):
                data, (b_, h_, w_) = model(img, lowres=True)
                lo = TokenMap(data, b_, h_, w_)
            else:
                lo = core.forward_lowres(img)
            if named_loss is not None:
                loss = named_loss(lo, lbl)
            else:
                loss = criterion_lowres(lo, lbl, img.shape[2:], loss_weight, num_classes=args.nb_classes, dice=args.dice,
                                        ignore_index=args.ignore_index)
        elif named_loss is not None:
            loss = named_loss(model(img), lbl)
        else:
            loss = criterion(model(img), lbl, loss_weight, num_classes=args.nb_classes, dice=args.dice,
                             ignore_index=args.ignore_index)
        loss_value = loss.item()
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping training".format(loss_value))
            sys.exit(1)
        is_second_order = hasattr(optimizer, 'is_second_order') and optimizer.is_second_order
        loss_scaler(loss, optimizer, clip_grad=clip_grad, clip_mode=clip_mode, parameters=model.parameters(),
                    create_graph=is_second_order)
        lr = optimizer.param_groups[0]["lr"]
        metric_logger.update(loss=loss_value, lr=lr)
        if writer is not None and idx % print_freq == 0 and getattr(args, 'local_rank', 0) == 0:
            it = epoch * num_steps + idx
            writer.add_scalar('train_loss', loss, it)
            writer.add_scalar('train_lr', lr, it)
    if pending is not None and pending.n:           # a loader that yielded fewer batches than len() promised
        _flush_losses(pending, metric_logger, writer if getattr(args, 'local_rank', 0) == 0 else None, print_freq, epoch * num_steps)
    metric_logger.synchronize_between_processes()
    return metric_logger.meters["loss"].global_avg, lr


EVAL_DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


MSF_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def msf_sizes(H, W, scales, multiple=32):
    """Network input size per scale of a multi-scale evaluation: the scaled size, each side rounded UP to a multiple of the model
    stride -- (ceil(int(s H) / multiple) multiple, ceil(int(s W) / multiple) multiple), as semseg's evaluate_msf does."""
    return [(int(math.ceil(int(s * H) / multiple)) * multiple, int(math.ceil(int(s * W) / multiple)) * multiple) for s in scales]


@torch.inference_mode()
def evaluate_msf(args, model, dataloader, device, print_freq, writer=None, scales=MSF_SCALES, flip=True):
    """Multi-scale + flip evaluation (the protocol behind the published mIoU figures; semseg's evaluate_msf): every batch runs
    through the model at each of `scales` (sizes: msf_sizes), with `flip` also horizontally mirrored; the class probabilities of all
    those outputs, resized to the label size, are summed and the arg max of the sum is scored.  Returns (confmat, metric) like
    `evaluate`, with the same eval-dtype switch, buffer broadcast and reductions.  The resize of the 3-channel input is a torch op (tiny
    next to the forward); everything after the forwards is ONE kernel per batch (Metrics.update_msf): no full-resolution logits or
    probability map exists.

    Aliasing: a GraphedEvalSession replays one graph per input shape and hands back that graph's STATIC output buffer.  The straight
    and the mirrored forward of one scale share a shape, so the second replay would overwrite the first result before update_msf
    reads it: the straight result is copied into a buffer kept per shape for the whole evaluation (no allocation per step)."""
    model.eval()
    metric = Metrics(args.nb_classes, args.ignore_label, device)
    confmat = utils.ConfusionMatrix(args.nb_classes)
    metric_logger = utils.MetricLogger(delimiter="  ")
    core = model.module if hasattr(model, 'module') else model
    fused = hasattr(core, 'forward_lowres')
    eval_dtype = EVAL_DTYPES[str(getattr(args, 'eval_dtype', None) or 'fp32')]
    trained_dtype = getattr(core, 'compute_dtype', None)
    switch = hasattr(core, 'set_compute_dtype') and trained_dtype is not None and trained_dtype != eval_dtype
    if switch:
        core.set_compute_dtype(eval_dtype)
    try:
        return _evaluate_msf(args, model, core, fused, dataloader, device, print_freq, writer, metric, confmat, metric_logger,
                             tuple(scales), bool(flip))
    finally:
        if switch:
            core.set_compute_dtype(trained_dtype)


def _evaluate_msf(args, model, core, fused, dataloader, device, print_freq, writer, metric, confmat, metric_logger, scales, flip):
    if not scales or len(scales) * (2 if flip else 1) > hip.MSF_MAX_MAPS:
        raise ValueError(f'evaluate_msf: 1 .. {hip.MSF_MAX_MAPS} maps per image ({len(scales)} scales, flip={flip})')
    if utils.get_world_size() > 1:
        from .graph import broadcast_buffers_
        broadcast_buffers_(core)                                  # as _evaluate: the forwards below bypass the DDP wrapper
    session = None
    graph_pref = getattr(args, 'hip_graph', None)
    if (graph_pref is None or bool(graph_pref)) and fused and torch.device(device).type == 'cuda':
        from .graph import GraphedEvalSession
        # one graph per scale (straight and mirrored share it); room for every scale of this call
        session = GraphedEvalSession(core, max_graphs=max(8, len(scales)), max_captures=max(8, len(scales)))
    kept = {}                                                     # (shape, dtype) -> copy of the straight result (see the docstring)

    def forward(x):
        if fused:
            return session(x) if (session is not None and x.is_cuda) else core.forward_lowres(x)
        out = model(x)
        return tokens_from_nchw(out, out.dtype if out.dtype in (torch.float32, torch.bfloat16) else torch.float32)

    for idx, (images, labels) in enumerate(metric_logger.log_every(dataloader, print_freq, 'Test (MSF):')):
        images = images.to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)
        H, W = images.shape[2:]
        maps, flips = [], []
        for size in msf_sizes(H, W, scales):
            x = images if size == (H, W) else torch.nn.functional.interpolate(images, size=size, mode='bilinear', align_corners=False)
            lo = forward(x)
            if flip and session is not None and x.is_cuda:
                key = (tuple(lo.data.shape), lo.data.dtype)
                buf = kept.get(key)
                if buf is None:
                    buf = kept[key] = torch.empty_like(lo.data)
                buf.copy_(lo.data)
                lo = TokenMap(buf, lo.B, lo.H, lo.W)
            maps.append(lo)
            flips.append(0)
            if flip:
                maps.append(forward(x.flip(3)))
                flips.append(1)
        metric.update_msf(maps, flips, labels, (H, W), confmat=confmat)      # one pass: every map, both matrices
        if writer and idx % print_freq == 0:
            writer.add_scalar('valid_mf1', metric.compute_f1()[1])
            writer.add_scalar('valid_acc', metric.compute_pixel_acc()[1])
            writer.add_scalar('valid_mIOU', metric.compute_iou()[1])
    confmat.reduce_from_all_processes()
    metric.reduce_from_all_processes()
    return confmat, metric


def slide_windows(H, W, crop, stride):
    """Window grid of a sliding-window evaluation over an H x W image (mmseg's slide_inference; segf_slide_grid of include/segfac.h):
    -> (crop_eff, stride_eff, [(y, x), ...]) in window order (rows of windows, then columns).  The crop is clamped to the image,
    crop_eff = (min(ch, H), min(cw, W)), and the stride to the crop, stride_eff = min(stride, crop_eff) per axis; an axis has
    max(L - crop + stride - 1, 0) // stride + 1 windows, window i at min(i stride, L - crop): the last one is moved back to end at the
    border."""
    (ch, cw), (sh, sw) = hip.hw_pair(crop, 'crop'), hip.hw_pair(stride, 'stride')
    if min(H, W, ch, cw, sh, sw) < 1:
        raise ValueError(f'slide_windows: sizes must be positive (image {H} x {W}, crop {ch} x {cw}, stride {sh} x {sw})')
    ch, cw = min(ch, H), min(cw, W)
    sh, sw = min(sh, ch), min(sw, cw)
    ys = [min(i * sh, H - ch) for i in range(max(H - ch + sh - 1, 0) // sh + 1)]
    xs = [min(j * sw, W - cw) for j in range(max(W - cw + sw - 1, 0) // sw + 1)]
    return (ch, cw), (sh, sw), [(y, x) for y in ys for x in xs]


def default_slide_stride(crop):
    """floor(2 crop / 3) per axis, at least 1: 512 -> 341, 1024 -> 682."""
    ch, cw = hip.hw_pair(crop, 'crop')
    return max(2 * ch // 3, 1), max(2 * cw // 3, 1)


@torch.inference_mode()
def evaluate_slide(args, model, dataloader, device, print_freq, writer=None, crop=512, stride=None, window_batch=None):
    """Sliding-window evaluation (mmseg's slide_inference, the protocol behind SegFormer's Cityscapes figures and most ADE20K / VOC
    configurations): every image is cut into overlapping `crop` windows at `stride` (slide_windows; stride None: floor(2 crop / 3)), the
    model runs on the windows, the logits of overlapping windows -- each resized to the crop -- are averaged and the arg max of the mean
    is scored.  Returns (confmat, metric) like `evaluate`, with the same eval-dtype switch, buffer broadcast and reductions.  The
    windows are torch slices of the 3-channel input; everything after the forwards is ONE kernel per batch (Metrics.update_slide): no
    full-resolution logits, accumulator or count map exists.

    window_batch None: all B nWin windows of a batch go through one forward.  An integer: chunks of at most that many; their outputs
    land in ONE buffer kept per shape for the whole evaluation (no allocation per step).  Aliasing (as in evaluate_msf): chunks share a
    shape, hence a graph of the GraphedEvalSession, hence its STATIC output buffer -- each chunk is copied out before the next replay."""
    model.eval()
    metric = Metrics(args.nb_classes, args.ignore_label, device)
    confmat = utils.ConfusionMatrix(args.nb_classes)
    metric_logger = utils.MetricLogger(delimiter="  ")
    core = model.module if hasattr(model, 'module') else model
    fused = hasattr(core, 'forward_lowres')
    eval_dtype = EVAL_DTYPES[str(getattr(args, 'eval_dtype', None) or 'fp32')]
    trained_dtype = getattr(core, 'compute_dtype', None)
    switch = hasattr(core, 'set_compute_dtype') and trained_dtype is not None and trained_dtype != eval_dtype
    if switch:
        core.set_compute_dtype(eval_dtype)
    try:
        return _evaluate_slide(args, model, core, fused, dataloader, device, print_freq, writer, metric, confmat, metric_logger,
                               hip.hw_pair(crop, 'crop'), hip.hw_pair(stride, 'stride') if stride is not None else default_slide_stride(crop),
                               window_batch)
    finally:
        if switch:
            core.set_compute_dtype(trained_dtype)


def _evaluate_slide(args, model, core, fused, dataloader, device, print_freq, writer, metric, confmat, metric_logger, crop, stride,
                    window_batch):
    if window_batch is not None and int(window_batch) < 1:
        raise ValueError(f'evaluate_slide: window_batch must be at least 1, got {window_batch}')
    if utils.get_world_size() > 1:
        from .graph import broadcast_buffers_
        broadcast_buffers_(core)                                  # as _evaluate: the forwards below bypass the DDP wrapper
    session = None
    graph_pref = getattr(args, 'hip_graph', None)
    if (graph_pref is None or bool(graph_pref)) and fused and torch.device(device).type == 'cuda':
        from .graph import GraphedEvalSession
        session = GraphedEvalSession(core)                        # one graph per chunk shape (full chunks and the remainder)
    kept = {}                                                     # (rows, columns, dtype) -> the windows' buffer (see the docstring)

    def forward(x):
        if fused:
            return session(x) if (session is not None and x.is_cuda) else core.forward_lowres(x)
        out = model(x)
        return tokens_from_nchw(out, out.dtype if out.dtype in (torch.float32, torch.bfloat16) else torch.float32)

    for idx, (images, labels) in enumerate(metric_logger.log_every(dataloader, print_freq, 'Test (slide):')):
        images = images.to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)
        B = images.shape[0]
        H, W = images.shape[2:]
        (ch, cw), strd, origins = slide_windows(H, W, crop, stride)
        n = B * len(origins)
        # image-major, then window order: the layout segf_slide_argmax_confmat reads
        x = torch.stack([images[:, :, y:y + ch, x0:x0 + cw] for y, x0 in origins], dim=1).reshape(n, images.shape[1], ch, cw)
        if window_batch is None or int(window_batch) >= n:
            lo = forward(x)
            windows = (lo.data, lo.H, lo.W)
        else:
            buf = None
            for k in range(0, n, int(window_batch)):
                lo = forward(x[k:k + int(window_batch)])
                per = lo.H * lo.W                                 # rows per window
                if buf is None:
                    key = (n * per, lo.data.shape[1], lo.data.dtype)
                    buf = kept.get(key)
                    if buf is None:
                        buf = kept[key] = torch.empty((n * per, lo.data.shape[1]), dtype=lo.data.dtype, device=lo.data.device)
                buf[k * per:k * per + lo.data.shape[0]].copy_(lo.data)        # out of the graph's static buffer before the next replay
            windows = (buf, lo.H, lo.W)
        metric.update_slide(windows, labels, (H, W), (ch, cw), strd, confmat=confmat)     # one pass: every window, both matrices
        if writer and idx % print_freq == 0:
            writer.add_scalar('valid_mf1', metric.compute_f1()[1])
            writer.add_scalar('valid_acc', metric.compute_pixel_acc()[1])
            writer.add_scalar('valid_mIOU', metric.compute_iou()[1])
    confmat.reduce_from_all_processes()
    metric.reduce_from_all_processes()
    return confmat, metric


@torch.inference_mode()
def evaluate_msf_slide(args, model, dataloader, device, print_freq, writer=None, scales=MSF_SCALES, flip=True, crop=512, stride=None,
                       window_batch=None):
    """Multi-scale + flip sliding-window evaluation (mmseg's aug_test with mode='slide', the protocol behind SegFormer's multi-scale
    Cityscapes figures): every batch is resized to each of `scales` (sizes: msf_sizes), with `flip` also horizontally mirrored; each
    of those images is cut into overlapping `crop` windows at `stride` (slide_windows on the scaled size; stride None: floor(2 crop /
    3)), the model runs on the windows, the logits of overlapping windows are averaged, the mean is resized to the label size and
    softmaxed, the probabilities of all (scale, flip) pairs are summed and the arg max of the sum is scored.  Returns (confmat, metric)
    like `evaluate`, with the same eval-dtype switch, buffer broadcast and reductions.  The resize and the window slices of the
    3-channel input are torch ops; everything after the forwards is ONE kernel per batch (Metrics.update_msf_slide): no
    full-resolution logits, accumulator, count map or probability map exists, at the label size or at a scaled size.

    window_batch None: all B nWin windows of a (scale, flip) pair go through one forward.  An integer: chunks of at most that many.
    Aliasing (wider than in evaluate_msf / evaluate_slide): a GraphedEvalSession replays one graph per input shape and hands back that
    graph's STATIC output buffer, and the full-size windows of ALL scales, straight and mirrored, share one shape.  Every forward's
    result is therefore copied into its slot of a buffer kept per (set index, shape) for the whole evaluation (no allocation per step
    after the first batch of a shape) before the next replay."""
    model.eval()
    metric = Metrics(args.nb_classes, args.ignore_label, device)
    confmat = utils.ConfusionMatrix(args.nb_classes)
    metric_logger = utils.MetricLogger(delimiter="  ")
    core = model.module if hasattr(model, 'module') else model
    fused = hasattr(core, 'forward_lowres')
    eval_dtype = EVAL_DTYPES[str(getattr(args, 'eval_dtype', None) or 'fp32')]
    trained_dtype = getattr(core, 'compute_dtype', None)
    switch = hasattr(core, 'set_compute_dtype') and trained_dtype is not None and trained_dtype != eval_dtype
    if switch:
        core.set_compute_dtype(eval_dtype)
    try:
        return _evaluate_msf_slide(args, model, core, fused, dataloader, device, print_freq, writer, metric, confmat, metric_logger,
                                   tuple(scales), bool(flip), hip.hw_pair(crop, 'crop'),
                                   hip.hw_pair(stride, 'stride') if stride is not None else default_slide_stride(crop), window_batch)
    finally:
        if switch:
            core.set_compute_dtype(trained_dtype)


def _evaluate_msf_slide(args, model, core, fused, dataloader, device, print_freq, writer, metric, confmat, metric_logger, scales, flip,
                        crop, stride, window_batch):
    if not scales or len(scales) * (2 if flip else 1) > hip.MSF_MAX_MAPS:
        raise ValueError(f'evaluate_msf_slide: 1 .. {hip.MSF_MAX_MAPS} window sets per image ({len(scales)} scales, flip={flip})')
    if window_batch is not None and int(window_batch) < 1:
        raise ValueError(f'evaluate_msf_slide: window_batch must be at least 1, got {window_batch}')
    if utils.get_world_size() > 1:
        from .graph import broadcast_buffers_
        broadcast_buffers_(core)                                  # as _evaluate: the forwards below bypass the DDP wrapper
    session = None
    graph_pref = getattr(args, 'hip_graph', None)
    if (graph_pref is None or bool(graph_pref)) and fused and torch.device(device).type == 'cuda':
        from .graph import GraphedEvalSession
        # per scale at most a clamped crop, hence a chunk shape and a remainder shape of its own
        session = GraphedEvalSession(core, max_graphs=max(8, 2 * len(scales)), max_captures=max(8, 2 * len(scales)))
    kept = {}                                                     # (set index, rows, columns, dtype) -> that set's windows (see the docstring)

    def forward(x):
        if fused:
            return session(x) if (session is not None and x.is_cuda) else core.forward_lowres(x)
        out = model(x)
        return tokens_from_nchw(out, out.dtype if out.dtype in (torch.float32, torch.bfloat16) else torch.float32)

    def run_windows(k, x):
        """Head outputs of the windows x of set k as (rows, h, w): one forward, or chunks of window_batch, each copied out of the
        graph's static buffer into the set's own buffer before the next replay."""
        n = x.shape[0]
        step = n if window_batch is None else min(int(window_batch), n)
        if step == n and not (session is not None and x.is_cuda):
            lo = forward(x)                                       # eager and whole: a fresh tensor, nothing to alias
            return lo.data, lo.H, lo.W
        buf = None
        for a in range(0, n, step):
            lo = forward(x[a:a + step])
            per = lo.H * lo.W                                     # rows per window
            if buf is None:
                key = (k, n * per, lo.data.shape[1], lo.data.dtype)
                buf = kept.get(key)
                if buf is None:
                    buf = kept[key] = torch.empty((n * per, lo.data.shape[1]), dtype=lo.data.dtype, device=lo.data.device)
            buf[a * per:a * per + lo.data.shape[0]].copy_(lo.data)
        return buf, lo.H, lo.W

    for idx, (images, labels) in enumerate(metric_logger.log_every(dataloader, print_freq, 'Test (slide-MSF):')):
        images = images.to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)
        B = images.shape[0]
        H, W = images.shape[2:]
        sets, flips = [], []
        for size in msf_sizes(H, W, scales):
            xs = images if size == (H, W) else torch.nn.functional.interpolate(images, size=size, mode='bilinear', align_corners=False)
            (ch, cw), strd, origins = slide_windows(size[0], size[1], crop, stride)
            for f in ((0, 1) if flip else (0,)):
                src = xs.flip(3) if f else xs
                # image-major, then window order: the layout segf_msf_slide_argmax_confmat reads
                x = torch.stack([src[:, :, y:y + ch, x0:x0 + cw] for y, x0 in origins], dim=1).reshape(B * len(origins), src.shape[1], ch, cw)
                sets.append((run_windows(len(sets), x), size, (ch, cw), strd))
                flips.append(f)
        metric.update_msf_slide(sets, flips, labels, (H, W), confmat=confmat)      # one pass: every set, both matrices
        if writer and idx % print_freq == 0:
            writer.add_scalar('valid_mf1', metric.compute_f1()[1])
            writer.add_scalar('valid_acc', metric.compute_pixel_acc()[1])
            writer.add_scalar('valid_mIOU', metric.compute_iou()[1])
    confmat.reduce_from_all_processes()
    metric.reduce_from_all_processes()
    return confmat, metric


@torch.inference_mode()
def evaluate(args, model, dataloader, device, print_freq, writer=None):
    """engine.py:74-104.  The reference evaluates in fp32 with autocast deliberately off (engine.py:86-88), whatever precision it
    trained in -- so does this: the forward runs the exact-fp32 kernels unless `args.eval_dtype == 'bf16'` (train_gpu.py
    --eval-dtype bf16: the production storage type, ~5x the rate; tests/test_model_gpu.py measures what it flips).
    `args.eval_scales` (non-empty) or `args.eval_flip` hand the call to evaluate_msf; without them nothing here changes.
    `args.eval_mode == 'slide'` hands it to evaluate_slide (args.eval_crop, default args.image_size; args.eval_stride, default
    floor(2 crop / 3); args.eval_window_batch); in that mode sliding windows at several scales or mirrored are not built: ValueError.
    `args.eval_mode == 'slide-msf'` is the mode that has them: evaluate_msf_slide, crop / stride / window batch read as in 'slide',
    scales / flip as for evaluate_msf."""
    if getattr(args, 'eval_mode', 'whole') == 'slide-msf':
        crop = getattr(args, 'eval_crop', None) or getattr(args, 'image_size', None)
        if crop is None:
            raise ValueError("evaluate: eval_mode 'slide-msf' needs args.eval_crop (or args.image_size)")
        return evaluate_msf_slide(args, model, dataloader, device, print_freq, writer,
                                  scales=tuple(getattr(args, 'eval_scales', None) or (1.0,)), flip=bool(getattr(args, 'eval_flip', False)),
                                  crop=crop, stride=getattr(args, 'eval_stride', None),
                                  window_batch=getattr(args, 'eval_window_batch', None))
    if getattr(args, 'eval_mode', 'whole') == 'slide':
        scales = tuple(getattr(args, 'eval_scales', None) or (1.0,))
        if scales != (1.0,) or getattr(args, 'eval_flip', False):
            raise ValueError("evaluate: eval_mode 'slide' with eval_scales other than (1.0,) or with eval_flip -- sliding windows at "
                             "several scales or mirrored are not built in this mode; use eval_mode 'slide-msf'")
        crop = getattr(args, 'eval_crop', None) or getattr(args, 'image_size', None)
        if crop is None:
            raise ValueError("evaluate: eval_mode 'slide' needs args.eval_crop (or args.image_size)")
        return evaluate_slide(args, model, dataloader, device, print_freq, writer, crop=crop, stride=getattr(args, 'eval_stride', None),
                              window_batch=getattr(args, 'eval_window_batch', None))
    if getattr(args, 'eval_scales', None) or getattr(args, 'eval_flip', False):
        return evaluate_msf(args, model, dataloader, device, print_freq, writer,
                            scales=tuple(getattr(args, 'eval_scales', None) or (1.0,)), flip=bool(getattr(args, 'eval_flip', False)))
    model.eval()
    metric = Metrics(args.nb_classes, args.ignore_label, device)
    confmat = utils.ConfusionMatrix(args.nb_classes)
    metric_logger = utils.MetricLogger(delimiter="  ")
    header = 'Test:'
    core = model.module if hasattr(model, 'module') else model
    fused = hasattr(core, 'forward_lowres')
    eval_dtype = EVAL_DTYPES[str(getattr(args, 'eval_dtype', None) or 'fp32')]
    trained_dtype = getattr(core, 'compute_dtype', None)
    switch = hasattr(core, 'set_compute_dtype') and trained_dtype is not None and trained_dtype != eval_dtype
    if switch:
        core.set_compute_dtype(eval_dtype)
    try:
        return _evaluate(args, model, core, fused, dataloader, device, print_freq, writer, metric, confmat, metric_logger, header)
    finally:
        if switch:
            core.set_compute_dtype(trained_dtype)


def _evaluate(args, model, core, fused, dataloader, device, print_freq, writer, metric, confmat, metric_logger, header):
    if utils.get_world_size() > 1:
        # collective C2: the reference evaluates the DDP-wrapped model, whose forward first hands every rank rank 0's BatchNorm
        # buffers (train_gpu.py:233-236, broadcast_buffers=True).  The forwards below call the core module directly (graph path: there
        # is no wrapper at all), so the broadcast is issued here, once, in front of the forwards that read the running statistics
        from .graph import broadcast_buffers_
        broadcast_buffers_(core)
    session = None
    graph_pref = getattr(args, 'hip_graph', None)            # None = auto (on), as in train_one_epoch
    if (graph_pref is None or bool(graph_pref)) and fused and torch.device(device).type == 'cuda':
        from .graph import GraphedEvalSession
        session = GraphedEvalSession(core)                   # the eval forward as a replayed hipGraph per RECURRING input shape
    for idx, (images, labels) in enumerate(metric_logger.log_every(dataloader, print_freq, header)):
        images = images.to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)
        if fused:
            lo = session(images) if (session is not None and images.is_cuda) else core.forward_lowres(images)
            metric.update_lowres(lo, labels, images.shape[2:], confmat=confmat)     # one pass feeds both matrices
        else:
            outputs = model(images)
            confmat.update(labels.flatten(), outputs.argmax(1).flatten())
            metric.update(outputs, labels.flatten())
        if writer and idx % print_freq == 0:
            writer.add_scalar('valid_mf1', metric.compute_f1()[1])
            writer.add_scalar('valid_acc', metric.compute_pixel_acc()[1])
            writer.add_scalar('valid_mIOU', metric.compute_iou()[1])
    confmat.reduce_from_all_processes()
    metric.reduce_from_all_processes()
    return confmat, metric
