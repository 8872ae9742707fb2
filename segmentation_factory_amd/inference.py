"""Single-image inference: the GPU half of the reference's ``estimate_model.py`` (class SemSeg, :53-123).

    preprocess   (estimate_model.py:85-98)   short side -> img_size, ceil to a multiple of 32, /255, ImageNet normalise
    model_forward(:113-115)                  SegmentationModel under inference_mode
    postprocess  (:100-111)                  logits -> F.interpolate(orig size, bilinear, align_corners=True)
                                             -> softmax(dim=1).argmax(dim=1) -> palette

File reading, the dataset palettes / class names and ``draw_text`` stay with the reference's ``datasets`` package (PIL /
torchvision, outside the hot path: SURVEY section 8); this module takes and returns tensors.  The device work -- model, the two
bilinear resizes (head -> network input size with align_corners=False as build_models.py:65 does, then -> original size with
align_corners=True) and the class arg max -- runs in the HIP library: the low-resolution head output is the only logits tensor
that exists in bf16; both resizes run in fp32 on NHWC rows and the arg max reads the final rows directly (softmax is monotonic,
so it is skipped).
"""
import math

import torch

from . import hip
from .backbones import TokenMap

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class SemSeg:
    def __init__(self, model, img_size=1024, palette=None, labels=None, device='cuda'):
        """model: a segmentation_factory_amd.SegmentationModel with its weights loaded (the reference loads 'model_state' /
        'state_dict' checkpoints into the same keys).  palette: optional uint8 tensor [num_classes, 3]."""
        self.device = device
        self.model = model.to(device).eval()
        self.size = [img_size, img_size]
        self.palette = palette.to(device) if palette is not None else None
        self.labels = labels

    def inference_size(self, H, W):
        """estimate_model.py:88-92: scale the short side to the target, then up to the next multiple of the model stride."""
        scale = self.size[0] / min(H, W)
        nH, nW = round(H * scale), round(W * scale)
        return int(math.ceil(nH / 32)) * 32, int(math.ceil(nW / 32)) * 32

    def preprocess(self, image: torch.Tensor) -> torch.Tensor:
        """image: uint8 CHW in [0, 255] -> normalised fp32 [1, 3, nH, nW] on the device: estimate_model.py:85-97 as ONE kernel of this
        library (segf_infer_preprocess: T.Resize of a uint8 tensor as torchvision 0.15.2 computes it -- bilinear, no antialias, rounded
        back to uint8 -- then / 255 and mean / std)."""
        H, W = image.shape[1:]
        nH, nW = self.inference_size(H, W)
        if image.dtype != torch.uint8:
            # the reference feeds torchvision.io.read_image's uint8 tensor (estimate_model.py:117-118), and T.Resize of a uint8 tensor
            # rounds back to uint8 where a float tensor would be interpolated in float: silently rounding a float image here would
            # match neither.  Only the byte path is pinned (byte-equal to torch's CPU resize), so only it is accepted
            raise TypeError(f'SemSeg.preprocess takes the uint8 CHW image torchvision.io.read_image returns, got {image.dtype}')
        img = image.to(self.device).contiguous()
        mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=self.device)
        std = torch.tensor(IMAGENET_STD, dtype=torch.float32, device=self.device)
        return hip.infer_preprocess(img, nH, nW, mean, std)

    @torch.inference_mode()
    def model_forward(self, img: torch.Tensor) -> TokenMap:
        """Head output at stride 4 as NHWC token rows (the full-resolution logits tensor is formed in postprocess)."""
        return self.model.forward_lowres(img)

    def _colour(self, seg, orig_img, overlay):
        """Palette image of a [1, H0, W0] segmentation map (None without a palette), optionally blended over the original image."""
        if self.palette is None:
            return None
        img = self.palette[seg].squeeze(0)
        if overlay and orig_img is not None:
            img = orig_img.to(img.device).permute(1, 2, 0) * 0.4 + img * 0.6
        return img

    @torch.inference_mode()
    def postprocess(self, orig_hw, lo: TokenMap, in_hw, orig_img=None, overlay=False):
        """-> (seg_map int64 [H0, W0], colour image uint8/float [H0, W0, 3] or None)."""
        B, h, w = lo.B, lo.H, lo.W
        nc = self.model.num_classes if hasattr(self.model, 'num_classes') else lo.data.shape[1]
        H1, W1 = in_hw
        H0, W0 = orig_hw
        ld = (nc + 7) // 8 * 8
        low = torch.zeros((B * h * w, ld), dtype=torch.float32, device=lo.data.device)
        hip.cast2d(lo.data[:, :nc], low[:, :nc])                                   # bf16 head output -> fp32 rows
        mid = torch.empty((B * H1 * W1, ld), dtype=torch.float32, device=low.device)
        hip.bilinear_fwd(low, B, h, w, ld, H1, W1, mid, align_corners=False)        # build_models.py:65
        full = torch.empty((B * H0 * W0, ld), dtype=torch.float32, device=low.device)
        hip.bilinear_fwd(mid, B, H1, W1, ld, H0, W0, full, align_corners=True)      # estimate_model.py:102
        seg = hip.argmax_rows(full, nc).view(B, H0, W0)                             # :104
        return seg.squeeze(0), self._colour(seg, orig_img, overlay)

    @torch.inference_mode()
    def msf_maps(self, x: torch.Tensor, scales, flip: bool):
        """Head outputs of the preprocessed image x at every scale (engine.msf_sizes of x's size), each also for the mirrored
        input when `flip`: ([TokenMap], [flip flag]) in the order the probabilities are summed."""
        from .engine import msf_sizes
        H1, W1 = x.shape[2:]
        maps, flips = [], []
        for size in msf_sizes(H1, W1, scales):
            xs = x if size == (H1, W1) else torch.nn.functional.interpolate(x, size=size, mode='bilinear', align_corners=False)
            maps.append(self.model_forward(xs))
            flips.append(0)
            if flip:
                maps.append(self.model_forward(xs.flip(3)))
                flips.append(1)
        return maps, flips

    @torch.inference_mode()
    def postprocess_msf(self, orig_hw, maps, flips, orig_img=None, overlay=False):
        """Multi-scale + flip prediction: every map resampled to the original size (bilinear, align_corners=False), softmaxed and
        summed, arg max of the sum -- one kernel (hip.msf_argmax_confmat without labels), its pred_out is the segmentation map."""
        H0, W0 = orig_hw
        B = maps[0].B
        nc = self.model.num_classes if hasattr(self.model, 'num_classes') else maps[0].data.shape[1]
        seg = torch.empty((B, H0, W0), dtype=torch.int64, device=maps[0].data.device)
        hip.msf_argmax_confmat(maps, flips, B, nc, H0, W0, None, -1, None, None, None, pred_out=seg)
        return seg.squeeze(0), self._colour(seg, orig_img, overlay)

    @torch.inference_mode()
    def predict_slide(self, x: torch.Tensor, orig_hw, crop, stride, orig_img=None, overlay=False):
        """Sliding-window prediction of the preprocessed image x: the model runs on the overlapping windows of engine.slide_windows
        (crop clamped to x), the windows' logits are averaged and the arg max of the mean is taken -- one kernel
        (hip.slide_argmax_confmat without labels), its pred_out is the segmentation map at x's size; an original size that differs is
        reached by nearest-neighbour lookup of the class indices."""
        from .engine import default_slide_stride, slide_windows
        B, _, H1, W1 = x.shape
        (ch, cw), strd, origins = slide_windows(H1, W1, crop, stride if stride is not None else default_slide_stride(crop))
        xs = torch.stack([x[:, :, y:y + ch, x0:x0 + cw] for y, x0 in origins], dim=1).reshape(B * len(origins), x.shape[1], ch, cw)
        lo = self.model_forward(xs)
        nc = self.model.num_classes if hasattr(self.model, 'num_classes') else lo.data.shape[1]
        seg = torch.empty((B, H1, W1), dtype=torch.int64, device=lo.data.device)
        hip.slide_argmax_confmat(lo, B, nc, H1, W1, (ch, cw), strd, None, -1, None, None, None, pred_out=seg)
        H0, W0 = orig_hw
        if (H0, W0) != (H1, W1):
            iy = (torch.arange(H0, device=seg.device) * H1) // H0
            ix = (torch.arange(W0, device=seg.device) * W1) // W0
            seg = seg[:, iy][:, :, ix]
        return seg.squeeze(0), self._colour(seg, orig_img, overlay)

    @torch.inference_mode()
    def predict_msf_slide(self, x: torch.Tensor, orig_hw, crop, stride, scales, flip, orig_img=None, overlay=False):
        """Multi-scale + flip sliding-window prediction of the preprocessed image x: at every scale (engine.msf_sizes of x's size),
        straight and -- with `flip` -- mirrored, the model runs on the overlapping windows of engine.slide_windows of the scaled image;
        per (scale, flip) pair the windows' logits are averaged, the mean is resampled to x's size and softmaxed, the probabilities
        are summed and the arg max of the sum is taken -- one kernel (hip.msf_slide_argmax_confmat without labels), its pred_out is
        the segmentation map at x's size; an original size that differs is reached by nearest-neighbour lookup of the class indices,
        as in predict_slide."""
        from .engine import default_slide_stride, msf_sizes, slide_windows
        B, _, H1, W1 = x.shape
        stride = stride if stride is not None else default_slide_stride(crop)
        sets, flips = [], []
        for size in msf_sizes(H1, W1, tuple(scales) if scales else (1.0,)):
            xs = x if size == (H1, W1) else torch.nn.functional.interpolate(x, size=size, mode='bilinear', align_corners=False)
            (ch, cw), strd, origins = slide_windows(size[0], size[1], crop, stride)
            for f in ((0, 1) if flip else (0,)):
                src = xs.flip(3) if f else xs
                win = torch.stack([src[:, :, y:y + ch, x0:x0 + cw] for y, x0 in origins], dim=1).reshape(B * len(origins), x.shape[1], ch, cw)
                sets.append((self.model_forward(win), size, (ch, cw), strd))
                flips.append(f)
        lo = sets[0][0]
        nc = self.model.num_classes if hasattr(self.model, 'num_classes') else lo.data.shape[1]
        seg = torch.empty((B, H1, W1), dtype=torch.int64, device=lo.data.device)
        hip.msf_slide_argmax_confmat(sets, flips, B, nc, H1, W1, None, -1, None, None, None, pred_out=seg)
        H0, W0 = orig_hw
        if (H0, W0) != (H1, W1):
            iy = (torch.arange(H0, device=seg.device) * H1) // H0
            ix = (torch.arange(W0, device=seg.device) * W1) // W0
            seg = seg[:, iy][:, :, ix]
        return seg.squeeze(0), self._colour(seg, orig_img, overlay)

    def predict(self, image: torch.Tensor, overlay: bool = True, scales=None, flip: bool = False, slide=None, msf_slide=None):
        """image: uint8 CHW tensor (what torchvision.io.read_image returns).  -> (seg_map, colour image or None).
        scales (e.g. (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)) and / or flip: multi-scale + flip prediction (postprocess_msf); slide =
        (crop, stride) (stride None: floor(2 crop / 3)): sliding-window prediction (predict_slide), not together with scales / flip;
        msf_slide = (crop, stride): sliding windows at every one of `scales` (default (1.0,)) and, with `flip`, mirrored
        (predict_msf_slide), not together with slide; without them the single forward of the reference."""
        if msf_slide is not None and slide is not None:
            raise ValueError('SemSeg.predict: msf_slide together with slide -- give one of them')
        if slide is not None and (scales or flip):
            raise ValueError('SemSeg.predict: slide together with scales / flip -- sliding windows at several scales or mirrored are '
                             'not built for slide=; use msf_slide=(crop, stride)')
        x = self.preprocess(image)
        if msf_slide is not None:
            crop, stride = msf_slide
            return self.predict_msf_slide(x, tuple(image.shape[1:]), crop, stride, tuple(scales) if scales else (1.0,), bool(flip), image,
                                          overlay)
        if slide is not None:
            crop, stride = slide
            return self.predict_slide(x, tuple(image.shape[1:]), crop, stride, image, overlay)
        if scales or flip:
            maps, flips = self.msf_maps(x, tuple(scales) if scales else (1.0,), bool(flip))
            return self.postprocess_msf(tuple(image.shape[1:]), maps, flips, image, overlay)
        lo = self.model_forward(x)
        return self.postprocess(tuple(image.shape[1:]), lo, tuple(x.shape[2:]), image, overlay)
