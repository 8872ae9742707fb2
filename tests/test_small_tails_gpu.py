"""The two single-workgroup tails of the step, bernoulli_scale_kernel (DropPath / Dropout2d scales) and ce_dice_loss_kernel (the loss
finalize): both issue their loads in batches, neither may move a bit.  The scales are checked against a numpy restatement of the
counter generator, the loss against float64 arithmetic on the statistics the kernel read."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


def _splitmix64(z):
    """numpy uint64 restatement of splitmix64 (wrap-around arithmetic)."""
    with np.errstate(over='ignore'):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _scales_ref(seed, ctr, kp, n, row_len):
    with np.errstate(over='ignore'):
        base = _splitmix64(np.array([seed ^ ((ctr * 0xD1B54A32D192ED03) & M64)], dtype=np.uint64))
        i = np.arange(n, dtype=np.uint64)
        r = _splitmix64(base + i)
    u = (r >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    k = kp[(np.arange(n, dtype=np.int64) // row_len)]
    return np.where(u < k, np.float32(1.0) / k, np.float32(0.0)).astype(np.float32)


@pytest.mark.parametrize('n,row_len', [(3 * 768, 768), (1 << 20, 4099), (3 * 768, 1 << 40), (1000, 1)],
                         ids=['3x768', '2^20-rows-of-4099', 'row-longer-than-table', 'row-of-one'])
def test_bernoulli_scale_is_the_counter_generator_bit_for_bit(n, row_len):
    """out[i] = U_i < kp[i // row_len] ? 1 / kp : 0 with U_i from splitmix64(splitmix64(seed ^ ctr * K) + i): every element equal to the
    numpy restatement over two launches, and the launch counter advances by one per launch."""
    from segmentation_factory_amd import hip
    rows = (n + row_len - 1) // row_len
    g = np.random.default_rng(5)
    kp = (0.05 + 0.95 * g.random(rows)).astype(np.float32)
    kp[0] = np.float32(0.9)
    seed, ctr0 = 0x1234_5678_9ABC_DEF1, 41
    state = torch.tensor([seed, ctr0], dtype=torch.int64, device='cuda')
    kpd = torch.from_numpy(kp).cuda()
    for launch in range(2):
        out = hip.bernoulli_scale(state, kpd, n, row_len).cpu().numpy()
        want = _scales_ref(seed, ctr0 + launch, kp, n, row_len)
        bad = int((out.view(np.uint32) != want.view(np.uint32)).sum())
        print(f'n={n} row_len={row_len} launch {launch}: {bad} unequal, kept {int((out != 0).sum())} of {n}')
        assert bad == 0
        assert state.cpu().tolist() == [seed, ctr0 + launch + 1]
    assert 0 < (out != 0).sum() < n or n < 8


@pytest.mark.parametrize('B', [2, 256, 300])
def test_loss_finalize_against_float64(B):
    """loss[3] = {ce + dice, ce, dice} of segf_ce_dice_fwd against float64 arithmetic on the per-sample statistics the finalize read
    (B x C = 2 x 150 and 256 x 150; 300 x 150 takes the second 256-sample chunk of the staged tail sums): 1e-6 relative; the four tail sums it
    leaves behind the table are the column sums."""
    from segmentation_factory_amd import hip
    C, h, w, H, W = 150, 4, 4, 16, 16
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(B * h * w, C, generator=g) * 2).to(torch.bfloat16).cuda()
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.1] = 255
    loss, stats = hip.ce_dice_fwd(logits, B, C, h, w, H, W, target.cuda(), 255, None, True)
    torch.cuda.synchronize()
    st = stats[:B * (3 * C + 4)].view(B, 3 * C + 4).double().cpu().numpy()
    eps = float(np.float32(1e-6))
    I, P, T, tail = st[:, :C], st[:, C:2 * C], st[:, 2 * C:3 * C], st[:, 3 * C:]
    sets = P + T
    sets = np.where(sets == 0.0, 2.0 * I, sets)
    dl = 1.0 - ((2.0 * I + eps) / (sets + eps)).mean()
    ts = tail.sum(axis=0)
    ce = ts[0] / ts[1]
    got = loss.double().cpu().numpy()
    for name, a, b in (('total', got[0], ce + dl), ('ce', got[1], ce), ('dice', got[2], dl)):
        print(f'B={B} {name}: kernel {a:.9f} float64 {b:.9f} rel {abs(a - b) / abs(b):.2e}')
        assert abs(a - b) <= 1e-6 * abs(b)
    got_tail = stats[B * (3 * C + 4):B * (3 * C + 4) + 4].double().cpu().numpy()
    assert np.all(np.abs(got_tail - ts) <= 1e-6 * np.abs(ts) + 1e-30), (got_tail, ts)
