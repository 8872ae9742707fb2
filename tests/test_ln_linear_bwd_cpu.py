"""Host side of the fused `LayerNorm -> Linear` backward (segf_layernorm_linear_bwd, ln_linear_bwd_kernel): the shape / size / policy rule,
the kernels a call launches, and the summation order of the C = 64 data gradient restated in scalar arithmetic -- without a GPU."""
import numpy as np
import pytest
import torch

BF16, F32 = torch.bfloat16, torch.float32
B4 = [(4 * 128 * 128, 32, 128), (4 * 64 * 64, 64, 256)]          # cfg2 (SegFormer-B0, 512^2) at batch 4: stages 1 and 2 (rows, C, hidden)
B256 = [(256 * 128 * 128, 32, 128), (256 * 64 * 64, 64, 256)]


def test_supported_follows_shape_size_and_policy(monkeypatch):
    from segmentation_factory_amd import hip
    sup = hip.layernorm_linear_bwd_supported
    assert hip.policy('ln_linear_bwd_fused') == 1
    for s in B4:
        assert not sup(BF16, *s), s                                # the recorded batch-4 step stays on its three launches
    for s in B256:
        assert sup(BF16, *s), s
        assert not sup(F32, *s), s
    assert sup(BF16, 131072, 32, 128) and not sup(BF16, 131071, 32, 128)
    assert not sup(BF16, 256 * 32 * 32, 160, 640) and not sup(BF16, 256 * 16 * 16, 256, 1024)      # stages 3 / 4
    assert not sup(BF16, 1 << 22, 32, 64) and not sup(BF16, 1 << 22, 64, 128) and not sup(BF16, 1 << 22, 32, 256)      # hidden != 4 C
    monkeypatch.setenv('SEGFAC_LN_LINEAR_BWD_FUSED', '0')
    for s in B4 + B256:
        assert not sup(BF16, *s), s
    monkeypatch.setenv('SEGFAC_LN_LINEAR_BWD_FUSED', '2')
    for s in B4 + B256 + [(37, 32, 128), (64, 64, 256)]:
        assert sup(BF16, *s), s
        assert not sup(F32, *s), s
    assert not sup(BF16, 256 * 32 * 32, 160, 640) and not sup(BF16, 1 << 22, 32, 64)
    assert not sup(BF16, 0, 32, 128)


@pytest.mark.parametrize('shape,ks', [(B256[0], 1), (B256[1], 2), ((1620, 32, 128), 1), ((37, 64, 256), 2)])
def test_dry_run_names_the_kernel_and_the_finalizes(shape, ks):
    from segmentation_factory_amd import dispatch, hip
    rows, Cc, N = shape
    lib, p = hip.lib(), dispatch._PLACEHOLDER
    nblk = lib.segf_layernorm_linear_bwd_blocks(rows)
    assert nblk == min((rows + 63) // 64, 512)
    assert lib.segf_layernorm_linear_bwd_ws(rows, Cc, N) == nblk * (N * Cc + N + 2 * Cc)
    for now in (False, True):
        outs = [p + 0x900, p + 0xa00, p + 0xb00, p + 0xb00 + 4 * Cc] if now else [None] * 4
        with hip.trace(dry_run=True) as t:
            rc = lib.segf_layernorm_linear_bwd(hip.BF16, rows, Cc, N, p, p + 0x100, p + 0x200, p + 0x300, p + 0x400, p + 0x500, p + 0x600,
                                               p + 0x700, p + 0x800, p + 0xc00, 16384, p + 0xd00, None, *outs, p + 0xe00, None)
        assert rc == 0
        assert len(t.kernels) == (4 if now else 1), t.kernels
        assert t.kernels[0].startswith(f'ln_linear_bwd_kernel<{ks}>'), t.kernels
        assert all(k.startswith('colreduce_finalize') for k in t.kernels[1:]), t.kernels


def test_entry_point_is_replayable_and_refuses_what_it_has_no_kernel_for():
    from segmentation_factory_amd import dispatch, hip
    lib, p = hip.lib(), dispatch._PLACEHOLDER
    assert dispatch._replayable('segf_layernorm_linear_bwd') and dispatch._replayable('segf_layernorm_linear_bwd_supported')

    def call(dt, rows, Cc, N, rscale=None, dxs=None, outs=(None,) * 4):
        with hip.trace(dry_run=True):
            return lib.segf_layernorm_linear_bwd(dt, rows, Cc, N, p, p, p, p, None, p, p, p, p, rscale, 1, dxs, None, *outs, p, None)
    assert call(hip.BF16, 4096, 32, 128) == 0
    assert call(hip.F32, 4096, 32, 128) != 0                       # fp32 storage: an error, not another path
    assert call(hip.BF16, 4096, 160, 640) != 0 and call(hip.BF16, 4096, 32, 64) != 0
    assert call(hip.BF16, 4096, 32, 128, rscale=p) != 0            # a scale without the scaled output
    assert call(hip.BF16, 4096, 32, 128, outs=(p, p, p, p)) != 0   # dbeta must follow dgamma
    assert call(hip.BF16, 4096, 32, 128, outs=(p, p, p, p + 128)) == 0
    # a recorded call replays as a dry run like every other
    entry = {'fn': 'segf_layernorm_linear_bwd',
             'args': [hip.BF16, 1 << 22, 32, 128] + ['p0'] * 9 + [None, 1, None, None, None, None, None, None, 'p0', None]}
    ks = dispatch.replay(entry)
    assert len(ks) == 1 and ks[0].startswith("ln_linear_bwd_kernel<1>"), ks


def _bf16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def k_quarter_dy(dh_row, w1):
    """fc1's data gradient of one token at C = 64 in the order gemm_skinny_k_kernel<1, 2, 4> and ln_linear_bwd_kernel<2> form it:
    the 256 hidden features in four quarters of 64, each quarter an accumulator that starts from zero and takes its two 32-wide
    matrix-instruction steps in ascending order, the four partials added as ((p0 + p1) + p2) + p3 in fp32, one rounding to bf16.
    (A 32-wide step is restated as its exact sum rounded once: the inputs below make every step exact.)"""
    dh_row, w1 = np.asarray(dh_row, np.float64), np.asarray(w1, np.float64)
    parts = []
    for q in range(4):
        acc = np.zeros(w1.shape[1], np.float32)
        for s in range(2):
            k = slice(64 * q + 32 * s, 64 * q + 32 * s + 32)
            acc = (acc.astype(np.float64) + dh_row[k] @ w1[k]).astype(np.float32)
        parts.append(acc)
    total = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    return _bf16(total)


def order_probe():
    """(dh row, W1 [256][64]) with one non-zero product per 32-wide step at most, so that every step is exact and only the order of
    the fp32 additions decides the result:
      column 0: quarter partials 2^24, 1, -2^24, 1        -> ((p0 + p1) + p2) + p3 = 1
      column 1: quarter partials 1, 2^24, 1, -2^24        -> 0   (pairs (p0 + p1) + (p2 + p3) would give 1)
      column 2: 2^24 | 1 in each step of quarter 1 | -2^24 | 0  -> 2   (ONE chain over all eight steps would give 0)"""
    dh_row = np.zeros(256, np.float32)
    w1 = np.zeros((256, 64), np.float32)
    big = 2.0 ** 24
    for q, (a, b, c) in enumerate(((big, 1.0, big), (1.0, big, 1.0), (-big, 1.0, -big), (1.0, -big, 0.0))):
        dh_row[64 * q + 5] = 1.0
        w1[64 * q + 5, :3] = (a, b, c)
    dh_row[64 + 32 + 7] = 1.0                                      # second step of quarter 1
    w1[64 + 32 + 7, 2] = 1.0
    return dh_row, w1


def test_k_quarter_order_restated_in_scalar_arithmetic():
    dh_row, w1 = order_probe()
    dy = k_quarter_dy(dh_row, w1)
    assert dy[0] == 1.0 and dy[1] == 0.0 and dy[2] == 2.0 and not dy[3:].any()
    # the same operands in other association orders give other answers: the probe tells the orders apart
    step = [[np.float32(dh_row[32 * s:32 * s + 32] @ w1[32 * s:32 * s + 32, c]) for s in range(8)] for c in range(3)]
    quarter = [[np.float32(st[2 * q] + st[2 * q + 1]) for q in range(4)] for st in step]
    assert (quarter[1][0] + quarter[1][1]) + (quarter[1][2] + quarter[1][3]) == 1.0
    chain = np.float32(0)
    for v in step[2]:
        chain = np.float32(chain + v)
    assert chain == 0.0
    # on ordinary data the restatement is the float64 product to within the fp32 partial sums and the one bf16 rounding
    rng = np.random.default_rng(3)
    dh_row = _bf16(rng.standard_normal(256))
    w1 = _bf16(rng.standard_normal((256, 64)) * 0.2)
    exact = dh_row.astype(np.float64) @ w1.astype(np.float64)
    got = k_quarter_dy(dh_row, w1).astype(np.float64)
    assert np.all(np.abs(got - exact) <= np.abs(exact) * 2.0 ** -8 + 2.0 ** -20)
