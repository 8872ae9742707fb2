"""The classifier's bias gradient riding on pass 1 of the fused BatchNorm backward (segf_bn_cls_bwd_full_db, bn_cls_bwd_kernel<1, KS,
false, true, true>): every other output bit-equal to segf_bn_cls_bwd_full, the bias gradient against the float64 column sum of the same
bf16 class gradients with the error of the column-sum launch it replaces as the yardstick."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (samples, rows per sample): 8208 rows = 513 sixteen-token groups per sample (odd: every chunk plan leaves a dead tail group)
GEOMS = [(2, 8208), (1, 16384)]


def _inputs(B, rps, C, K):
    g = torch.Generator().manual_seed(23)
    M = B * rps
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    dy = (torch.randn(M, K, generator=g) * 1e-2).to(torch.bfloat16)
    # +1 in the last row of every sample (the row a dead tail group is clamped to), -1 in the first: a dead row that counted, or a row
    # of the neighbouring sample, moves a sum by a whole number
    for b in range(B):
        dy[(b + 1) * rps - 1] = 1.0
        dy[b * rps] = -1.0
    w = (torch.randn(K, C, generator=g) / C ** 0.5).to(torch.bfloat16)
    gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    mean, var = x.float().mean(0), x.float().var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    drop = (torch.rand(B, C, generator=g) > 0.1).float() / 0.9
    x1 = (torch.randn(M, 32, generator=g) * 0.7).to(torch.bfloat16)
    return dy, w, x, mean, rstd, gam, bet, drop, x1


@pytest.mark.parametrize('with_x1', [False, True], ids=['plain', 'x1'])
@pytest.mark.parametrize('K', [32, 160, 192])
@pytest.mark.parametrize('C', [256, 768])
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: f'{g[0]}x{g[1]}')
def test_bias_gradient_rides_and_nothing_else_moves(geom, C, K, with_x1, monkeypatch):
    from segmentation_factory_amd import hip
    B, rps = geom
    M = B * rps
    monkeypatch.setenv('SEGFAC_HEAD_DB_RIDE', '2')
    if with_x1 and not hip.bn_cls_bwd_dw_supported(torch.bfloat16, M, C, K, rps, 32):
        assert K > 160                     # the stage-1 rider of pass 2 exists up to K = 160: nothing to pair the new entry point with
        return
    assert hip.bn_cls_bwd_full_db_supported(torch.bfloat16, M, C, K, rps)
    dy, w, x, mean, rstd, gam, bet, drop, x1 = _inputs(B, rps, C, K)
    dev = [t.cuda() for t in (dy, w, x, mean, rstd, gam, bet)]
    args = (*dev, 1, drop.cuda(), rps, False)
    x1d = x1.cuda() if with_x1 else None
    ref = hip.bn_cls_bwd_full(*args, x1=x1d)
    with hip.trace() as t:
        got = hip.bn_cls_bwd_full_db(*args, x1=x1d)
    assert any('bn_cls_bwd_kernel' in k for k in t.kernels) and not any('colreduce_kernel' in k for k in t.kernels), t.kernels
    torch.cuda.synchronize()
    for name, a, b in zip(('dx', 'dgamma', 'dbeta', 'dG', 'dwcls'), got[:5], ref):
        if b is None:
            assert a is None, name
            continue
        print(f'{name}: unequal elements {(a != b).sum().item()}')
        assert torch.equal(a, b), name
    want = dy.double().sum(0)
    db_new = got[5].double().cpu()
    db_old = hip.colsum(dev[0]).double().cpu()
    e_new, e_old = (db_new - want).abs().max().item(), (db_old - want).abs().max().item()
    print(f'B={B} rps={rps} C={C} K={K} x1={with_x1}: |db - float64| riding {e_new:.3e}, colsum launch {e_old:.3e}')
    assert e_new < 0.5                      # no dead row, no neighbour's row
    assert e_new <= 2.0 * e_old
    assert torch.equal(hip.bn_cls_bwd_full_db(*args, x1=x1d)[5], got[5])      # fixed order: two runs agree to the bit


def test_default_policy_starts_at_131072_rows(monkeypatch):
    from segmentation_factory_amd import hip
    sup = hip.bn_cls_bwd_full_db_supported
    assert hip.policy('head_db_ride') == 1
    assert not sup(torch.bfloat16, 4 * 16384, 768, 160, 16384)          # the recorded batch-4 step keeps its column-sum launch
    assert sup(torch.bfloat16, 8 * 16384, 768, 160, 16384)
    assert not sup(torch.float32, 8 * 16384, 768, 160, 16384)
    monkeypatch.setenv('SEGFAC_HEAD_DB_RIDE', '0')
    assert not sup(torch.bfloat16, 256 * 16384, 768, 160, 16384)
    monkeypatch.setenv('SEGFAC_HEAD_DB_RIDE', '2')
    assert sup(torch.bfloat16, 16384, 768, 160, 16384)
