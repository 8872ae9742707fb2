"""Write tests/golden/pixel_loss_cases.npz from the imported reference (run where the reference is checked out; see
oracle/ref_shim.py):  python tools/make_pixel_loss_goldens.py

The reference's loss classes (util/losses.py: OhemCrossEntropy, FocalLoss, CrossEntropy) are run in fp32 on
F.interpolate(low, (H, W), bilinear, align_corners=False) of recorded low-resolution logits, as models/build_models.py:65 feeds them.
The fixture is data only; per case `<name>/<field>`:
  geom (B, C, h, w, H, W), low<i> fp32 [B, h, w, C] (one per member of a tuple), labels uint8 [B, H, W], weight fp32 [C] (when given),
  aux fp64 (the aux_weights used), params fp64 (thresh | alpha, gamma), loss fp64 (the reference's fp32 value), dlow<i> fp32 = d loss / d
  low<i> by autograd, and for OHEM branch (0 threshold / 1 top-k), n_min, n_hard (of member 0) and gap = min |ce - theta| over all pixels
  in float64 (tests/pixel_loss_refs.py).

A threshold-branch pixel that changes sides moves the mean by (mean - theta) / n_sel, which is not small, so the tool ASSERTS gap >= 1e-3
in the threshold-branch cases (the seed is advanced until that holds and the intended branch is taken; the seed used is recorded).  In
the top-k branch a swap of near-equal neighbours of kappa moves the mean by less than the CE-map error / n_min: no assertion needed.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import pixel_loss_refs as R   # noqa: E402

GEOMS = {'r4': (2, 19, 8, 12, 32, 48), 'r1': (2, 5, 24, 24, 24, 24)}
GAP = 1e-3
# (name, kind, inputs, class weights, members of the tuple, constructor extras)
CASES = (('ohem_thresh', 'ohem', 'plain', False, 1, {}),
         ('ohem_topk', 'ohem', 'confident', False, 1, {}),
         ('ohem_weighted', 'ohem', 'plain', True, 1, {}),
         ('ohem_tuple', 'ohem', 'plain', False, 2, {'aux_weights': [1, 0.4]}),
         ('focal_025_2', 'focal', 'plain', False, 1, {'alpha': 0.25, 'gamma': 2.0}),
         ('focal_default', 'focal', 'plain', False, 1, {}),
         ('ce_weighted', 'ce', 'plain', True, 1, {}))


def run_reference(ref, kind, lows, t, cw, extras):
    """(loss, [d loss / d low_i]) of the reference class on the upsampled NCHW logits, fp32."""
    H, W = t.shape[-2:]
    lows = [lo.clone().requires_grad_(True) for lo in lows]
    preds = tuple(F.interpolate(lo.permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False) for lo in lows)
    if kind == 'ohem':
        fn = ref.losses.OhemCrossEntropy(R.IGNORE, cw, **extras)
    elif kind == 'focal':
        fn = ref.losses.FocalLoss(**extras)
    else:
        fn = ref.losses.CrossEntropy(R.IGNORE, cw)
    loss = fn(preds if len(preds) > 1 else preds[0], t)
    loss.backward()
    return loss.detach(), [lo.grad for lo in lows]


def make_case(ref, name, kind, inp, weighted, members, extras, gname, geom, seed0):
    theta = R.theta_of(0.7)
    for seed in range(seed0, seed0 + 64):
        gen = R.plain_inputs if inp == 'plain' else R.confident_inputs
        pairs = [gen(geom, seed + 1000 * i) for i in range(members)]
        t = pairs[0][1]
        lows = [lo for lo, _ in pairs]
        cw = R.random_weights(geom[1], seed + 7) if weighted else None
        out = {'geom': np.array(geom, dtype=np.int64), 'labels': t.numpy().astype(np.uint8), 'seed': np.int64(seed)}
        if kind == 'ohem':
            ok = True
            for i, lo in enumerate(lows):
                sel = R.ohem(R.ce(lo, t, cw)[0], t, theta)
                gap = float((R.ce(lo, t, cw)[0] - theta).abs().min())
                if i == 0:
                    out.update(branch=np.int64(sel['used_topk']), n_min=np.int64(sel['n_min']), n_hard=np.int64(sel['n_hard']),
                               gap=np.float64(gap))
                ok = ok and sel['used_topk'] == (1 if inp == 'confident' else 0) and (sel['used_topk'] == 1 or gap >= GAP)
            if not ok:
                continue
            assert out['branch'] == 1 or out['gap'] >= GAP
        loss, grads = run_reference(ref, kind, lows, t, cw, extras)
        for i, (lo, gr) in enumerate(zip(lows, grads)):
            out[f'low{i}'] = lo.numpy()
            out[f'dlow{i}'] = gr.numpy()
        if cw is not None:
            out['weight'] = cw.numpy()
        out['aux'] = np.array(extras.get('aux_weights', [1.0]), dtype=np.float64)
        out['params'] = np.array([0.7] if kind == 'ohem' else [extras.get('alpha', 1), extras.get('gamma', 0)], dtype=np.float64)
        out['loss'] = np.float64(loss.item())
        print(f'[{name}_{gname}] seed {seed} loss {loss.item():.6f} ' +
              (f"branch {int(out['branch'])} n_min {int(out['n_min'])} n_hard {int(out['n_hard'])} gap {float(out['gap']):.4f}"
               if kind == 'ohem' else ''))
        return out
    raise AssertionError(f'{name}_{gname}: no seed in [{seed0}, {seed0 + 64}) gives the intended branch with a gap >= {GAP}')


def main():
    from oracle import ref_shim
    ref = ref_shim.load()
    flat = {}
    for gi, (gname, geom) in enumerate(GEOMS.items()):
        for ci, (name, kind, inp, weighted, members, extras) in enumerate(CASES):
            case = make_case(ref, name, kind, inp, weighted, members, extras, gname, geom, 100 + 100 * ci + 1000 * gi)
            for k, v in case.items():
                flat[f'{name}_{gname}/{k}'] = v
    path = R.golden_path()
    np.savez_compressed(path, **flat)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
