"""The float64 references of tests/attn_ref64.py checked against the oracle and against autograd, at small shapes (CPU only)."""
import math

import torch

import attn_ref64 as R
from oracle import flowtron_oracle as O


def _attn_inputs(T, B, Lk, A, seed, prior):
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn(T, B, A, generator=g, dtype=torch.float64) * 0.7
    K = torch.randn(Lk, B, A, generator=g, dtype=torch.float64) * 0.7
    v = torch.randn(A, generator=g, dtype=torch.float64) * 0.3
    lens = torch.randint(1, Lk + 1, (B,), generator=g)
    lens[0] = Lk
    pr = None
    if prior:
        pr = torch.rand(B, T, Lk, generator=g, dtype=torch.float64) ** 3
        pr[0, 0, 0] = 0.0
    return Q, K, v, lens, pr


def _oracle_attention(Q, K, v, lens, pr, temp):
    """oracle.attention with identity projections: queries = Q, keys = K, v = v"""
    A = Q.shape[2]
    eye = torch.eye(A, dtype=torch.float64)
    sd = {"query.linear_layer.weight": eye, "key.linear_layer.weight": eye, "value.linear_layer.weight": eye,
          "v.linear_layer.weight": v[None]}
    pad = ~(torch.arange(K.shape[0])[None, :] < lens[:, None])
    _, attn, logprob = O.attention(sd, "", Q, K, pad, pr, temperature=temp, chunk=4)
    return attn, logprob


def test_attention_forward_matches_oracle():
    for prior in (False, True):
        Q, K, v, lens, pr = _attn_inputs(9, 3, 7, 12, 1 + prior, prior)
        ref = R.attention_fwd(Q, K, v, lens, pr, 0.8)
        attn, logprob = _oracle_attention(Q, K, v, lens, pr, 0.8)
        if prior:   # the oracle takes log(prior + 1e-20) in fp32 (attn_prior.float()): its rounding, 2 U |log| per element
            lq = torch.log(pr.float().double() + 1e-20).abs()
            assert ((ref["logprob"] - logprob).abs() <= 2 * R.U * (lq + 1) + 1e-14).all()
            assert ((ref["attn"] - attn).abs() <= ref["attn"] * 4 * R.U * (lq.amax(2, keepdim=True) + 1) + 1e-15).all()
        else:
            assert (ref["attn"] - attn).abs().max() < 1e-14
            assert (ref["logprob"] - logprob).abs().max() < 1e-12
        for fn in (R.bound_p, R.bound_attn, R.bound_logprob):
            b = fn(ref)
            assert torch.isfinite(b).all() and (b >= 0).all()


def test_attention_backward_matches_autograd():
    temp = 0.8
    for prior in (False, True):
        for with_dlp in (False, True):
            Q, K, v, lens, pr = _attn_inputs(11, 3, 6, 10, 7 + 2 * prior + with_dlp, prior)
            Qg, Kg, vg = (t.clone().requires_grad_(True) for t in (Q, K, v))
            attn, logprob = _oracle_attention(Qg, Kg, vg, lens, pr, temp)
            g = torch.Generator().manual_seed(3)
            da = torch.randn(attn.shape, generator=g, dtype=torch.float64)
            valid = (torch.arange(K.shape[0])[None, :] < lens[:, None])[:, None, :]
            dl = torch.randn(attn.shape, generator=g, dtype=torch.float64) * 0.1 * valid if with_dlp else None
            loss = (attn * da).sum() + ((logprob * dl).sum() if with_dlp else 0.0)
            loss.backward()
            ref = R.attention_fwd(Q, K, v, lens, pr, temp, bounds=False)
            # (the oracle's own attn: its fp32 log(prior) is a constant of the graph, not an error of the backward)
            de, err = R.attention_de(attn.detach(), ref["p"], da, dl, lens, temp, prior=prior)
            assert torch.isfinite(err).all()
            gr = R.attention_grads(Q, K, v, lens, de)
            for mine, r in ((gr["dQ"], Qg.grad), (gr["dK"], Kg.grad), (gr["dv"], vg.grad)):
                assert (mine - r).abs().max() <= 1e-12 * (1 + r.abs().max()), (prior, with_dlp, (mine - r).abs().max())
            for k in ("dQ_err", "dK_err", "dv_err"):
                assert torch.isfinite(gr[k]).all() and (gr[k] >= 0).all()


def _ctc_inputs(B, T, Lk, seed):
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(B, T, Lk, generator=g, dtype=torch.float64) * 2, 2)
    return lp


def test_ctc_matches_torch_ctc_loss():
    B, T, Lk = 6, 17, 7
    lp = _ctc_inputs(B, T, Lk, 5)
    in_lens = torch.tensor([7, 5, 5, 3, 1, 6])
    out_lens = torch.tensor([17, 12, 5, 9, 3, 4])           # sample 2: T == K; sample 5: T < K (infeasible, zero_infinity)
    for blank in (-1.0, -8.0):
        x = lp.clone().requires_grad_(True)
        ref = O.attention_ctc_loss(x, in_lens, out_lens, blank_logprob=blank)
        (ref * 0.37).backward()
        mine = R.ctc_ref(lp, in_lens, out_lens, blank, gout=0.37)
        assert abs(mine["loss"].item() - ref.item()) < 1e-12 * abs(ref.item())
        assert (mine["grad"] - torch.nan_to_num(x.grad)).abs().max() < 1e-12
        assert not bool(mine["feasible"][5]) and float(mine["grad"][5].abs().max()) == 0.0
        for k in ("nll_err", "grad_err"):
            assert torch.isfinite(mine[k]).all() and (mine[k] >= 0).all()
        assert math.isfinite(float(mine["loss_err"]))
        # alpha / beta: sum_s exp(alpha + beta - em) at any frame equals the path probability, the same for every t
        b = 0
        a, be = mine["alpha"][b], mine["beta"][b]
        em = torch.full_like(a, -math.inf)
        lse = mine["lse"][b]
        em[:, 0::2] = blank - lse[:, None]
        em[:, 1::2] = lp[b] - lse[:, None]
        tot = torch.logsumexp(a + be - em, 1)[:17]
        assert (tot + mine["nll"][b]).abs().max() < 1e-10


def test_ctc_reads_no_padding():
    B, T, Lk = 3, 9, 5
    lp = _ctc_inputs(B, T, Lk, 8)
    in_lens, out_lens = torch.tensor([5, 3, 2]), torch.tensor([9, 6, 4])
    nan = lp.clone()
    for b in range(B):
        nan[b, out_lens[b]:] = float("nan")
        nan[b, :, in_lens[b]:] = float("nan")
    r0, r1 = R.ctc_ref(lp, in_lens, out_lens, -8.0), R.ctc_ref(nan, in_lens, out_lens, -8.0)
    assert torch.equal(r0["grad"], r1["grad"]) and torch.equal(r0["loss"], r1["loss"])


def test_ctc_multi_mirroring_is_flip_and_concatenate():
    B, T, Lk = 4, 13, 6
    in_lens, out_lens = torch.tensor([6, 4, 4, 2]), torch.tensor([13, 9, 7, 5])
    flows = [_ctc_inputs(B, T, Lk, 20 + f) for f in range(3)]
    flags = [1, 0, 1]
    stored = [R.mirror(x, out_lens, bool(r)) for x, r in zip(flows, flags)]      # each flow in its own time order
    # mirror twice is the identity; rows past T_b stay in place
    assert torch.equal(R.mirror(stored[0], out_lens), flows[0])
    assert torch.equal(stored[0][3, 5:], flows[0][3, 5:])
    multi = R.ctc_multi_ref(stored, flags, in_lens, out_lens, -8.0)
    # the oracle's FlowtronLoss: flip back the reversed flows, per-flow batch mean, mean over flows
    xs = [s.clone().requires_grad_(True) for s in stored]
    ctc = sum(O.attention_ctc_loss(O.reverse_by_length(x, out_lens, 1, 0) if r else x, in_lens, out_lens, -8.0)
              for x, r in zip(xs, flags)) / len(xs)
    ctc.backward()
    assert abs(multi["loss"].item() - ctc.item()) < 1e-12 * abs(ctc.item())
    for mine, x in zip(multi["grads"], xs):
        assert (mine - x.grad).abs().max() < 1e-12
    cat = R.ctc_ref(torch.cat(flows, 0), in_lens.repeat(3), out_lens.repeat(3), -8.0)
    assert torch.equal(cat["grad"], multi["grad"]) and abs(cat["loss"].item() - multi["loss"].item()) < 1e-15


def test_ctc_bound_grows_with_length():
    """the accumulated alpha / beta rounding bound is monotone in T_b (a bound that did not grow would not cover T 862)"""
    lp = _ctc_inputs(1, 60, 5, 2)
    errs = [float(R.ctc_ref(lp, torch.tensor([5]), torch.tensor([t]), -8.0)["nll_err"][0]) for t in (10, 30, 60)]
    assert errs[0] < errs[1] < errs[2]
