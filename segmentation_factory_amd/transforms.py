"""Device-side input pipeline: the reference's train / val transform stacks over decoded uint8 images resident in HBM.

Reference (datasets/build_datasets.py:14-29):
    train = ExtCompose([ExtRandomCrop((S, S)), ExtColorJitter(0.5, 0.5, 0.5), ExtRandomHorizontalFlip(), ExtToTensor(),
                        ExtNormalize(mean, std)])
    val   = ExtCompose([ExtResize(S), ExtToTensor(), ExtNormalize(mean, std)])
followed by the dataset class' label table and ``.long()`` (datasets/ade.py:122-124, cityscapes.py:159, coco_stuff.py:95-100,
voc.py:230).  There the stack runs per sample on PIL images inside DataLoader workers (about a hundred images per second and
core); here JPEG / PNG decoding stays wherever the caller does it, the decoded bytes are uploaded once (all of ADE20K is ~15 GB
of the 288 GB), and a batch is produced by two kernel launches (csrc/input.hip, `segf_input_train`) with Pillow's uint8
arithmetic reproduced bit for bit, including the second ``/ 255`` of ExtNormalize (quirk Q11).

The RANDOM DRAWS stay on the host and follow the reference's call order on Python's ``random`` module -- ExtRandomCrop.get_params
(extra_transform.py:342-360), ExtColorJitter.get_params (:470-497: brightness, contrast, saturation factor, then
``random.shuffle``), ExtRandomHorizontalFlip (:205-213) -- so that, with the same seed and the same decoded images, a batch equals
what the reference's single-process loader yields.  No CPU fallback: the tensors must be device tensors.

Scale augmentation (``DeviceTrainTransform(scale_range=, pad_if_needed=, label_fill=)``): ExtRandomScale (extra_transform.py:75-96)
and ExtRandomCrop(pad_if_needed=True) (:378-385) in front of the same stack, `segf_input_train_scaled` -- Pillow's resize evaluated
for the crop window only.

Class-balanced crop choice (``DeviceTrainTransform(cat_max_ratio=, crop_tries=, ignore_class=)``): mmsegmentation's
RandomCrop(crop_size, cat_max_ratio) in front of either stack.  The host draws ``crop_tries + 1`` candidate windows where it drew
one; which of them is used is decided on the device from the label histogram of each window (`segf_input_crop_select`,
`segf_input_train_scaled_select`; the rule is written out in include/segfac.h), because the labels live in HBM and a verdict read
back to the host would make the loader wait for the train step still in flight.
"""
import ctypes as C
import random as _random

import torch

from . import hip

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION = 1, 2, 3
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def label_table(mapping=None, device='cuda'):
    """int64[256] label table: identity, overridden by `mapping` {uint8 value: class id} (ADE20K: {255: 0}, datasets/ade.py:123;
    Cityscapes: id_to_train_id, cityscapes.py:159; COCO-Stuff: label_map, coco_stuff.py:98-100)."""
    t = torch.arange(256, dtype=torch.int64)
    for k, v in (mapping or {}).items():
        t[int(k)] = int(v)
    return t.to(device)


def _jitter_range(v):
    """ExtColorJitter._check_input (extra_transform.py:450-467) for brightness / contrast / saturation given as a number."""
    if v is None or v == 0:
        return None
    if isinstance(v, (tuple, list)):
        lo, hi = float(v[0]), float(v[1])
        if not 0 <= lo <= hi:
            raise ValueError(f'jitter range {v} should be between (0, inf)')
        return None if lo == hi == 1 else (lo, hi)
    if v < 0:
        raise ValueError('If a jitter amount is a single number, it must be non negative.')
    return (max(1.0 - v, 0.0), 1.0 + v)


class _Base:
    def __init__(self, mean, std, label_lut, device):
        self.device = torch.device(device)
        self.mean = torch.tensor(mean, dtype=torch.float32, device=self.device)
        self.std = torch.tensor(std, dtype=torch.float32, device=self.device)
        self.label_lut = None if label_lut is None else label_lut.to(self.device, torch.int64).contiguous()

    @staticmethod
    def _check(img, lbl):
        if not (img.is_cuda and lbl.is_cuda):
            raise RuntimeError('the device input pipeline needs device tensors (no CPU fallback)')
        if img.dtype != torch.uint8 or lbl.dtype != torch.uint8:
            raise TypeError('decoded images and labels must be uint8 (PIL RGB / L arrays)')
        if img.dim() != 3 or img.shape[2] != 3 or img.stride(2) != 1 or img.stride(1) != 3 or lbl.stride(-1) != 1 \
                or tuple(lbl.shape) != tuple(img.shape[:2]):
            raise ValueError(f'expected packed [h, w, 3] image and [h, w] label, got {tuple(img.shape)} / {tuple(lbl.shape)}')


class DeviceTrainTransform(_Base):
    """The training stack of build_datasets.py:14-22 for a whole batch.  ``rng``: a ``random.Random`` (default: the ``random``
    module itself, as the reference uses it).

    With ``scale_range=(lo, hi)`` the stack becomes the training protocol with scale augmentation,
        ExtCompose([ExtRandomScale((lo, hi)), ExtRandomCrop(size, pad_if_needed=...), ExtColorJitter, ExtRandomHorizontalFlip, ...])
    (extra_transform.py:75-96, 319-392): `draw_scaled` makes the draws and the size arithmetic, `segf_input_train_scaled` computes
    the crop window of the resized image without ever forming that image.  ``label_fill``: the raw uint8 label value of the
    border that ``pad_if_needed`` adds (the reference's F.pad fills 0; a training run wants its ignore label there).  Without
    ``scale_range`` and ``pad_if_needed`` nothing changes.

    With ``cat_max_ratio=R`` (0 < R < 1) the crop is mmseg's RandomCrop(size, cat_max_ratio=R): ``crop_tries + 1`` windows are drawn
    where one was (consecutive (row, column) pairs on the same stream, before the jitter factors), and the device takes the first
    of the first ``crop_tries`` in which no class covers R or more of the pixels whose class is not ``ignore_class`` and at least two
    classes occur, else the last one untested.  `last_chosen` is the device int32 [B] index of the window each sample of the last
    call took (0 for a sample that had one window only).  With ``cat_max_ratio`` None or >= 1 nothing changes."""

    def __init__(self, image_size, brightness=0.5, contrast=0.5, saturation=0.5, flip_p=0.5, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 label_lut=None, device='cuda', rng=None, scale_range=None, pad_if_needed=False, label_fill=0, cat_max_ratio=None,
                 crop_tries=10, ignore_class=255):
        super().__init__(mean, std, label_lut, device)
        self.size = (int(image_size), int(image_size)) if isinstance(image_size, (int, float)) else tuple(int(v) for v in image_size)
        self.ranges = [(OP_BRIGHTNESS, _jitter_range(brightness)), (OP_CONTRAST, _jitter_range(contrast)),
                       (OP_SATURATION, _jitter_range(saturation))]
        self.flip_p = flip_p
        self.rng = rng if rng is not None else _random
        if scale_range is not None:
            scale_range = (float(scale_range[0]), float(scale_range[1]))
            if not 0 < scale_range[0] <= scale_range[1]:
                raise ValueError(f'scale_range {scale_range} should be 0 < lo <= hi')
        if not 0 <= int(label_fill) <= 255:
            raise ValueError(f'label_fill {label_fill} is not a uint8 label value')
        self.scale_range, self.pad_if_needed, self.label_fill = scale_range, bool(pad_if_needed), int(label_fill)
        self.scaled = scale_range is not None or self.pad_if_needed
        if cat_max_ratio is not None and not cat_max_ratio > 0:
            raise ValueError(f'cat_max_ratio {cat_max_ratio} should be in (0, 1]')
        if not 1 <= int(crop_tries) <= 31:
            raise ValueError(f'crop_tries {crop_tries} should be 1 .. 31')
        self.balanced = cat_max_ratio is not None and cat_max_ratio < 1          # mmseg: `if self.cat_max_ratio < 1.`
        self.cat_max_ratio = float(cat_max_ratio) if self.balanced else None
        self.crop_tries, self.ignore_class = int(crop_tries), int(ignore_class)
        self.last_chosen = None

    def _jitter_flip(self):
        ops = [(op, self.rng.uniform(r[0], r[1])) for op, r in self.ranges if r is not None]
        self.rng.shuffle(ops)
        flip = self.rng.random() < self.flip_p
        return ops, bool(flip)

    def draw(self, src_h, src_w):
        """One sample's random values, drawn in the reference's order.  -> (top, left, [(op, factor), ...], flip)."""
        th, tw = self.size
        if src_w == tw and src_h == th:                     # ExtRandomCrop.get_params: no draw when the size already matches
            top, left = 0, 0
        else:
            top = self.rng.randint(0, abs(src_h - th))
            left = self.rng.randint(0, abs(src_w - tw))
        ops, flip = self._jitter_flip()
        return top, left, ops, flip

    def _windows(self, h, w):
        """The crop_tries + 1 candidate origins in an h x w image, (row, column) pairs drawn consecutively."""
        th, tw = self.size
        return [(self.rng.randint(0, abs(h - th)), self.rng.randint(0, abs(w - tw))) for _ in range(self.crop_tries + 1)]

    def draw_balanced(self, src_h, src_w):
        """`draw` for the class-balanced crop: -> (windows, [(op, factor), ...], flip) with windows = the crop_tries + 1 candidate
        (top, left) in drawing order, or the single (0, 0) when the source already has the crop's size (nothing is drawn then)."""
        th, tw = self.size
        windows = [(0, 0)] if src_w == tw and src_h == th else self._windows(src_h, src_w)
        ops, flip = self._jitter_flip()
        return windows, ops, flip

    @staticmethod
    def pad_border(res_h, res_w, th, tw):
        """ExtRandomCrop.__call__ with pad_if_needed (extra_transform.py:378-385): F.pad with an int pads ALL FOUR borders, first
        when the width is short, then -- on the already padded size -- when the height is.  -> the total border P."""
        p = 0
        if res_w < tw:
            p = int((1 + tw - res_w) / 2)
        if res_h + 2 * p < th:
            p += int((1 + th - (res_h + 2 * p)) / 2)
        return p

    def draw_scaled(self, src_h, src_w):
        """One sample's random values for the scaled stack, in the reference's order on the `random` stream: scale (:90), crop
        row, crop column (:359-360; none when the padded size equals the crop), the jitter factors, the shuffle, the flip.
        -> dict(scale, res_h, res_w, P, top, left, ops, flip, label_fill); (top, left) is the crop origin in the RESIZED image's
        coordinates (crop origin in the padded image minus P) and may be negative.  With ``cat_max_ratio`` the dict also has
        `windows`, the crop_tries + 1 candidate origins in drawing order (one when nothing is drawn), and (top, left) is the first."""
        th, tw = self.size
        scale = self.rng.uniform(self.scale_range[0], self.scale_range[1]) if self.scale_range is not None else None
        res_h, res_w = (src_h, src_w) if scale is None else (int(src_h * scale), int(src_w * scale))      # :91
        if res_h < 1 or res_w < 1:
            raise ValueError(f'scale {scale} leaves nothing of a {src_h} x {src_w} image')
        P = self.pad_border(res_h, res_w, th, tw) if self.pad_if_needed else 0
        hp, wp = res_h + 2 * P, res_w + 2 * P
        windows = None
        if wp == tw and hp == th:
            i, j = 0, 0
        elif self.balanced:
            windows = self._windows(hp, wp)
            i, j = windows[0]
        else:
            i = self.rng.randint(0, abs(hp - th))
            j = self.rng.randint(0, abs(wp - tw))
        ops, flip = self._jitter_flip()
        # without pad_if_needed a crop that hangs over the edge reads 0 in the label too (Image.crop)
        p = dict(scale=scale, res_h=res_h, res_w=res_w, P=P, top=i - P, left=j - P, ops=ops, flip=flip,
                 label_fill=self.label_fill if self.pad_if_needed else 0)
        if self.balanced:
            p['windows'] = [(a - P, b - P) for a, b in windows] if windows is not None else [(i - P, j - P)]
        return p

    def pack_scaled(self, images, labels, params):
        """-> (host array of segf_input_scaled_sample records, the largest tap count among them)."""
        recs = (hip.InputScaledSample * len(images))()
        kmax = 3
        for k, (img, lbl, p) in enumerate(zip(images, labels, params)):
            self._check(img, lbl)
            r = recs[k]
            r.img, r.lbl = img.data_ptr(), lbl.data_ptr()
            r.img_stride, r.lbl_stride = img.stride(0), lbl.stride(0)
            r.src_h, r.src_w, r.res_h, r.res_w = int(img.shape[0]), int(img.shape[1]), int(p['res_h']), int(p['res_w'])
            r.top, r.left, r.flip, r.label_fill = int(p['top']), int(p['left']), int(p['flip']), int(p['label_fill'])
            order = 0
            for j, (op, f) in enumerate(p['ops']):
                order |= op << (2 * j)
                r.factor[j] = f
            r.order = order
            if r.res_h >= 1 and r.res_w >= 1:               # (anything else is the library's to refuse)
                kmax = max(kmax, hip.resample_ksize(r.src_h, r.res_h), hip.resample_ksize(r.src_w, r.res_w))
        return recs, kmax

    def _candidates(self, windows):
        """Per-sample window lists -> (K, flat [B][K][2] int32 values); K = 1 when no sample has a choice, else crop_tries + 1 (a
        sample without a choice repeats its window: the kernel tests a repeated window once)."""
        K = max(len(w) for w in windows)
        if K > 1 and any(len(w) not in (1, K) for w in windows):
            raise ValueError('every sample needs one window or the same number of candidate windows')
        return K, [int(v) for w in windows for win in (w if len(w) == K else list(w) * K) for v in win]

    def _single_to_zero(self, windows, K):
        """A sample without a choice in a batch that has one: its repeated window is index 0, whatever the test said of it."""
        if any(len(w) != K for w in windows):
            keep = torch.tensor([int(len(w) == K) for w in windows], dtype=torch.int32).to(self.device)
            self.last_chosen.mul_(keep)                      # on the device: nothing is read back

    def pack(self, images, labels, params, cand=None):
        """-> the device records; with `cand` (flat [B][K][2] values) -> (records, int32 candidates) from ONE upload."""
        recs = (hip.InputSample * len(images))()
        for k, (img, lbl, (top, left, ops, flip)) in enumerate(zip(images, labels, params)):
            self._check(img, lbl)
            r = recs[k]
            r.img, r.lbl = img.data_ptr(), lbl.data_ptr()
            r.img_stride, r.lbl_stride = img.stride(0), lbl.stride(0)
            r.src_h, r.src_w, r.top, r.left = int(img.shape[0]), int(img.shape[1]), int(top), int(left)
            r.flip = int(flip)
            order = 0
            for j, (op, f) in enumerate(ops):
                order |= op << (2 * j)
                r.factor[j] = f                              # Python float -> C float, as Image.blend's (float)alpha
            r.order = order
        if cand is None:
            host = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8)
            return host.to(self.device, non_blocking=False)
        # the library cannot refuse these: the candidates of segf_input_crop_select stand on the device and are not read on the host
        if min(cand) < 0 or max(cand) > 1 << 30:
            raise ValueError('candidate windows of the unscaled stack must start inside [0, 2^30]')
        nrec = C.sizeof(recs)                                # a multiple of 8: the int32 candidates stand aligned behind the records
        dev = torch.frombuffer(bytearray(bytes(recs) + bytes((C.c_int32 * len(cand))(*cand))), dtype=torch.uint8).to(self.device)
        return dev[:nrec], dev[nrec:].view(torch.int32)

    def __call__(self, images, labels, params=None, out=None):
        """images: list of uint8 [h, w, 3] device tensors, labels: list of uint8 [h, w] -> (fp32 [B, 3, S, S], int64 [B, S, S]).
        ``params`` overrides the draws (one (top, left, ops, flip) per sample; with ``cat_max_ratio`` `draw_balanced`'s (windows, ops,
        flip) as well, and a sample given ONE window takes it without a test); ``out`` = (image, label) tensors to fill in place
        (e.g. the input buffers of a captured train step: zero-copy feed).  With ``scale_range`` / ``pad_if_needed`` the draws
        are `draw_scaled`'s dicts and the batch comes from `segf_input_train_scaled`."""
        oi, ol = out if out is not None else (None, None)
        B, (H, W) = len(images), self.size
        if self.scaled:
            if params is None:
                params = [self.draw_scaled(int(i.shape[0]), int(i.shape[1])) for i in images]
            wins = [p.get('windows') or [(p['top'], p['left'])] for p in params]
            K, cand = self._candidates(wins) if self.balanced else (1, None)
            recs, kmax = self.pack_scaled(images, labels, params)
            if K == 1:
                self.last_chosen = torch.zeros(B, dtype=torch.int32, device=self.device) if self.balanced else None
                return hip.input_train_scaled(recs, B, H, W, kmax, self.mean, self.std, self.label_lut, oi, ol)
            img, lbl, self.last_chosen = hip.input_train_scaled_select(
                recs, (C.c_int32 * len(cand))(*cand), B, K, H, W, kmax, self.cat_max_ratio, self.ignore_class, self.mean, self.std,
                self.label_lut, oi, ol)
            self._single_to_zero(wins, K)
            return img, lbl
        if not self.balanced:
            if params is None:
                params = [self.draw(int(i.shape[0]), int(i.shape[1])) for i in images]
            samples = self.pack(images, labels, params)
            return hip.input_train(samples, B, H, W, self.mean, self.std, self.label_lut, oi, ol)
        if params is None:
            params = [self.draw_balanced(int(i.shape[0]), int(i.shape[1])) for i in images]
        # `draw_balanced`'s (windows, ops, flip), or `draw`'s (top, left, ops, flip): a window without a choice
        params = [p if len(p) == 3 else ([(p[0], p[1])], p[2], p[3]) for p in params]
        K, cand = self._candidates([p[0] for p in params])
        first = [(p[0][0][0], p[0][0][1], p[1], p[2]) for p in params]
        if K == 1:
            self.last_chosen = torch.zeros(B, dtype=torch.int32, device=self.device)
            return hip.input_train(self.pack(images, labels, first), B, H, W, self.mean, self.std, self.label_lut, oi, ol)
        samples, dcand = self.pack(images, labels, first, cand)
        self.last_chosen = hip.input_crop_select(samples, dcand, B, K, H, W, self.cat_max_ratio, self.label_lut, self.ignore_class)
        self._single_to_zero([p[0] for p in params], K)
        return hip.input_train(samples, B, H, W, self.mean, self.std, self.label_lut, oi, ol)


class DeviceValTransform(_Base):
    """The validation stack of build_datasets.py:24-29 for one image (the resized size depends on the image)."""

    def __init__(self, image_size, mean=IMAGENET_MEAN, std=IMAGENET_STD, label_lut=None, device='cuda'):
        super().__init__(mean, std, label_lut, device)
        self.size = int(image_size)

    def output_size(self, src_h, src_w):
        """torchvision F.resize with an int: smaller edge -> size, the other int(size * long / short); unchanged when equal."""
        short, long_ = (src_w, src_h) if src_w <= src_h else (src_h, src_w)
        if short == self.size:
            return src_h, src_w
        new_long = int(self.size * long_ / short)
        return (new_long, self.size) if src_w <= src_h else (self.size, new_long)

    def __call__(self, img, lbl):
        self._check(img, lbl)
        oh, ow = self.output_size(int(img.shape[0]), int(img.shape[1]))
        return hip.input_val(img, lbl, oh, ow, self.mean, self.std, self.label_lut)


class DeviceDataset:
    """Decoded (image, label) pairs kept in HBM.  ``add`` takes what ``np.array(PIL image)`` gives (uint8 [h, w, 3] / [h, w])."""

    def __init__(self, device='cuda'):
        self.device = torch.device(device)
        self.images, self.labels = [], []

    def add(self, image, label):
        img = torch.as_tensor(image).contiguous()
        lbl = torch.as_tensor(label).contiguous()
        if img.dtype != torch.uint8 or lbl.dtype != torch.uint8:
            raise TypeError('decoded images and labels must be uint8')
        self.images.append(img.to(self.device))
        self.labels.append(lbl.to(self.device))

    def __len__(self):
        return len(self.images)


class DeviceBatchLoader:
    """Iterable of training batches for `engine.train_one_epoch`: what DataLoader(train_set, batch_size, drop_last=True,
    sampler=DistributedSampler / RandomSampler) over the transformed dataset yields (train_gpu.py:211-224), produced on the device.
    The index order is DistributedSampler's (torch/utils/data/distributed.py, drop_last=False): `randperm(n)` from a generator
    seeded `seed + epoch`, PADDED with its own head to `ceil(n / world) * world` entries, rank r taking entries r, r + world, ...;
    `set_epoch` reseeds as `sampler.set_epoch` does (train_gpu.py:323).  train_gpu.py's DistributedSampler is built without a
    seed, i.e. seed 0: pass seed=0 for its exact order.  (The single-process RandomSampler of the reference draws from torch's
    global generator instead; the same function with world=1 is used there -- same distribution, not the same sequence.)"""

    def __init__(self, dataset, batch_size, transform, shuffle=True, seed=0, rank=0, world=1):
        self.dataset, self.batch_size, self.transform = dataset, int(batch_size), transform
        self.shuffle, self.seed, self.rank, self.world, self.epoch = shuffle, seed, rank, world, 0
        self.out = None

    def bind_output(self, buffers):
        """From now on every batch is written into `buffers` = (image fp32 [B, 3, S, S], label int64 [B, S, S]) -- the input
        buffers of a captured train step (graph.GraphedTrainStep.static_inputs) -- and those tensors are what the loader yields:
        the step then has nothing to copy.  The consumer must be done with a batch before asking for the next (stream order
        guarantees it for the replayed step)."""
        img, lbl = buffers
        S = self.transform.size
        if tuple(img.shape) != (self.batch_size, 3, S[0], S[1]) or tuple(lbl.shape) != (self.batch_size, S[0], S[1]) \
                or img.dtype != torch.float32 or lbl.dtype != torch.int64 or not img.is_contiguous() or not lbl.is_contiguous():
            raise ValueError('bind_output: buffers do not match the batches of this loader')
        self.out = (img, lbl)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def num_samples(self):
        return -(-len(self.dataset) // self.world)             # ceil: DistributedSampler.num_samples with drop_last=False

    def __len__(self):
        return self.num_samples() // self.batch_size           # DataLoader(drop_last=True)

    def indices(self):
        """This rank's sample indices for the current epoch (DistributedSampler.__iter__)."""
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            order = torch.randperm(n, generator=g).tolist()
        else:
            order = list(range(n))
        total = self.num_samples() * self.world
        pad = total - len(order)
        if pad > 0:
            order += order[:pad] if pad <= len(order) else (order * (-(-pad // len(order))))[:pad]
        return order[self.rank:total:self.world]

    def __iter__(self):
        order = self.indices()
        for b in range(len(self)):
            idx = order[b * self.batch_size:(b + 1) * self.batch_size]
            yield self.transform([self.dataset.images[i] for i in idx], [self.dataset.labels[i] for i in idx], out=self.out)

