"""A launch ledger of the recurrence dispatch in flowtron_amd.ops: how many persistent (whole-chip) launches ops.PERSIST_LAUNCHES counts
around the forward and around the backward of ops.lstm_layer and ops.decoder_pair, at the smallest shapes that reach each path -- one
launch up to 32 batch rows, the roles kernels' slices above (128 rows forward, 64 backward), the zero-padded 1024-unit twin of a
narrower layer, and the decoder pair's pipelines (chunks + 1 launches) against its sequential backward (one launch per layer).
dist.py keeps collectives away from these launches by that counter, and a launch too many is ~T x 2 us of a whole chip."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.lib()
    if not ops.persist_usable(torch.device("cuda", 0)):          # (runs the self-test, whose own launches are then behind us)
        pytest.skip("persistent kernels not usable on this device")
    return L, ops


def _ledger(ops, forward, dh_shape):
    """(launches around forward(), launches around the backward of its result)"""
    n0 = ops.PERSIST_LAUNCHES
    h = forward()
    n1 = ops.PERSIST_LAUNCHES
    h.backward(torch.randn(dh_shape, generator=torch.Generator().manual_seed(5)).cuda() * 0.1)
    n2 = ops.PERSIST_LAUNCHES
    torch.cuda.synchronize()
    ops.check_persist_status()
    assert torch.isfinite(h).all()
    return n1 - n0, n2 - n1


@pytest.mark.parametrize("H,T,B,fwd,bwd", [(1024, 6, 5, 1, 1), (1024, 6, 40, 1, 1), (1024, 6, 130, 2, 3), (512, 64, 4, 1, 1)],
                         ids=["B5", "B40", "B130", "H512-padded"])
def test_lstm_layer_launches(env, H, T, B, fwd, bwd):
    L, ops = env
    gen = torch.Generator().manual_seed(1000 * B + H)
    K = 128
    x = (torch.randn(T, B, K, generator=gen) * 0.3).cuda().requires_grad_(True)
    w_ih, w_hh = [(torch.randn(4 * H, k, generator=gen) * 0.03).cuda().requires_grad_(True) for k in (K, H)]
    b_ih, b_hh = [(torch.randn(4 * H, generator=gen) * 0.03).cuda().requires_grad_(True) for _ in range(2)]
    lens = torch.randint(1, T + 1, (B,), generator=gen, dtype=torch.int32)
    lens[0] = T
    lens = lens.cuda()
    assert bool(ops.lstm_pad_width(B, H, False, L.FT_BF16, x.device, T)) == (H < 1024)
    assert ops.lstm_persist_groups(min(B, 32), 1024, False, L.FT_BF16, x.device)
    got = _ledger(ops, lambda: ops.lstm_layer(x, lens, w_ih, w_hh, b_ih, b_hh, mode=L.FT_BF16, rowmap=ops.row_map(lens, T, B)), (T, B, H))
    assert got == (fwd, bwd)
    assert all(torch.isfinite(t.grad).all() for t in (x, w_ih, w_hh, b_ih, b_hh))


@pytest.mark.parametrize("chunks_bwd,bwd", [(3, 4), (0, 2)], ids=["pipeline3", "sequential"])
def test_decoder_pair_launches(env, monkeypatch, chunks_bwd, bwd):
    L, ops = env
    T, B, K, H, chunks = 29, 5, 128, 1024, 4
    torch.manual_seed(11)
    p = torch.nn.LSTM(K, H, 2).cuda()
    gen = torch.Generator().manual_seed(B)
    x = (torch.randn(T, B, K, generator=gen) * 0.3).cuda().requires_grad_(True)
    lens = torch.tensor([7, 1, T, 8, 22], dtype=torch.int32).cuda()
    monkeypatch.setattr(ops, "_PAIR_CHUNKS_BWD", chunks_bwd)
    got = _ledger(ops, lambda: ops.decoder_pair(x, lens, p, L.FT_BF16, [], ops.row_map(lens, T, B), "dx", None, chunks)[0], (T, B, H))
    assert got == (chunks + 1, bwd)
    assert torch.isfinite(x.grad).all() and all(torch.isfinite(q.grad).all() for q in p.parameters())
