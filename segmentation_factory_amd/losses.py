"""The reference's loss classes (util/losses.py:9-66, 118-122) on the fused low-resolution loss path.

``forward(preds, labels)`` takes the stride-4 head output as a ``TokenMap`` (``model.forward_lowres(x)``; the full-resolution
size is ``labels.shape[-2:]`` and the final bilinear resize of build_models.py:65 happens inside the loss kernels), an NCHW
tensor of already full-resolution logits (``model(x)``), or a tuple of either with ``aux_weights``, as the reference does.
The full-resolution logits and their gradient are never formed on the ``TokenMap`` path, and nothing synchronises with the host:
OHEM's choice between its two branches is made on the device, so the losses run inside a captured train step.
"""
import math

import torch
from torch import nn

from . import functional as Fh
from .backbones import TokenMap

__all__ = ['CrossEntropy', 'OhemCrossEntropy', 'FocalLoss', 'get_loss']

_REFERENCE_NAMES = ['CrossEntropy', 'OhemCrossEntropy', 'Dice', 'FocalLoss']      # util/losses.py:6


def _as_lowres(pred, labels):
    """(token rows, geometry (B, C, h, w, H, W)) of one prediction."""
    H, W = labels.shape[-2:]
    if isinstance(pred, TokenMap):
        return pred.data, (pred.B, pred.data.shape[1], pred.H, pred.W, H, W)
    if not torch.is_tensor(pred) or pred.dim() != 4:
        raise TypeError(f'expected a TokenMap or a [B, C, H, W] tensor, got {type(pred).__name__}')
    B, C, h, w = pred.shape
    if (h, w) != (H, W):
        raise RuntimeError(f'NCHW predictions {tuple(pred.shape)} do not match labels {tuple(labels.shape)}')
    dtype = pred.dtype if pred.dtype in (torch.float32, torch.bfloat16) else torch.float32
    t = pred.permute(0, 2, 3, 1)
    if t.is_contiguous() and pred.dtype == dtype:
        rows = t.reshape(B * h * w, C)                      # zero-copy: already NHWC underneath
    else:
        rows = Fh.nchw_to_tokens(pred.to(dtype))
    return rows, (B, C, h, w, H, W)


class _PixelLoss(nn.Module):
    aux_weights = [1]
    weight = None

    def _weight_on(self, device):
        """fp32 class weights on `device`, converted once (a captured step must not meet a host-to-device copy)."""
        if self.weight is None:
            return None
        cache = self.__dict__.setdefault('_weight_cache', {})
        if device not in cache:
            cache[device] = torch.as_tensor(self.weight, dtype=torch.float32).to(device).contiguous()
        return cache[device]

    def _forward(self, pred, labels):
        raise NotImplementedError

    def forward(self, preds, labels):
        if isinstance(preds, tuple):
            return sum([w * self._forward(pred, labels) for (pred, w) in zip(preds, self.aux_weights)])
        return self._forward(preds, labels)


class CrossEntropy(_PixelLoss):
    """nn.CrossEntropyLoss(weight, ignore_index=ignore_label): the CE term of the fused CE + Dice kernels with dice off."""

    def __init__(self, ignore_label: int = 255, weight=None, aux_weights: list = [1, 0.4, 0.4]) -> None:
        super().__init__()
        self.ignore_label = ignore_label
        self.aux_weights = aux_weights
        self.weight = weight

    def _forward(self, pred, labels):
        rows, geom = _as_lowres(pred, labels)
        loss, _, _ = Fh.upsample_ce_dice(rows, labels, geom, self.ignore_label, self._weight_on(labels.device), False)
        return loss


class OhemCrossEntropy(_PixelLoss):
    """Online hard-example mining: the mean CE of the pixels with ce > -log(thresh), or of the n_valid // 16 largest when fewer
    than that many are hard.  ``thresh`` must lie in (0, 1): at thresh >= 1 the reference's threshold is <= 0 and it would count
    ignored pixels (ce == 0) as hard, so this class narrows the domain on purpose and raises ValueError.  Ties at the top-k cut
    share the gradient equally (include/segfac.h); the loss value is the reference's.  ``last_ce_map`` / ``last_info`` keep the
    newest call's per-pixel CE map and device-side counters (functional.pixel_loss_info reads them)."""

    def __init__(self, ignore_label: int = 255, weight=None, thresh: float = 0.7, aux_weights: list = [1, 1]) -> None:
        super().__init__()
        if not (0.0 < float(thresh) < 1.0):
            raise ValueError(f'OhemCrossEntropy: thresh must lie in (0, 1), got {thresh}')
        self.ignore_label = ignore_label
        self.aux_weights = aux_weights
        self.weight = weight
        # -torch.log(torch.tensor(thresh, dtype=torch.float)) of the reference: an fp32 value, compared in fp32
        self.thresh = float(-torch.log(torch.tensor(thresh, dtype=torch.float)))
        self.last_ce_map = self.last_info = None

    def _forward(self, pred, labels):
        rows, geom = _as_lowres(pred, labels)
        loss, self.last_ce_map, self.last_info = Fh.upsample_pixel_loss(
            rows, labels, geom, 'ohem', (self.thresh,), self.ignore_label, self._weight_on(labels.device))
        return loss


class FocalLoss(_PixelLoss):
    """alpha (1 - pt)^gamma ce with pt = exp(-ce), averaged over ALL pixels (ignored ones count in the divisor, as .mean() does)
    or summed (size_average=False).  Takes a single prediction or a tuple (weights 1), no class weights, any gamma >= 0."""

    def __init__(self, alpha=1, gamma=0, size_average=True, ignore_index=255):
        super().__init__()
        if not (float(gamma) >= 0.0 and math.isfinite(float(gamma))):
            raise ValueError(f'FocalLoss: gamma must be >= 0, got {gamma}')
        self.alpha = alpha
        self.gamma = gamma
        self.ignore_index = ignore_index
        self.size_average = size_average
        self.aux_weights = [1, 1, 1]
        self.last_ce_map = self.last_info = None

    def _forward(self, pred, labels):
        rows, geom = _as_lowres(pred, labels)
        loss, self.last_ce_map, self.last_info = Fh.upsample_pixel_loss(
            rows, labels, geom, 'focal', (self.alpha, self.gamma, self.size_average), self.ignore_index, None)
        return loss


def get_loss(loss_fn_name: str = 'CrossEntropy', ignore_label: int = 255, cls_weights=None):
    assert loss_fn_name in _REFERENCE_NAMES, \
        f"Unavailable loss function name >> {loss_fn_name}.\nAvailable loss functions: {_REFERENCE_NAMES}"
    if loss_fn_name == 'Dice':
        raise NotImplementedError(
            "get_loss('Dice'): the reference's Dice class applies no softmax to its input and cannot take an ignore label "
            "(F.one_hot raises on 255); the Dice term this library has is engine.criterion(dice=True).")
    if loss_fn_name == 'FocalLoss':
        raise NotImplementedError(
            "get_loss('FocalLoss'): the reference passes (ignore_label, cls_weights) into FocalLoss(alpha, gamma), which fails with "
            "a TypeError at the first forward; construct losses.FocalLoss(alpha, gamma, size_average, ignore_index) directly.")
    return {'CrossEntropy': CrossEntropy, 'OhemCrossEntropy': OhemCrossEntropy}[loss_fn_name](ignore_label, cls_weights)
