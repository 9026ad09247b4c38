"""Utterance scoring on the device (-m gpu): the likelihood kernel against its float64 replay (tests/score_ref.py) bit for bit,
alone and inside a batch, with NaN and 1e30 behind the lengths; the diagnostics kernel against integer logic on a float32
arg-max; infer_attention_maps against forced staircases; Flowtron.log_likelihood against the kernel on a direct forward,
FlowtronLoss and the CPU oracle; and the two use cases end to end."""
import os

import numpy as np
import pytest
import torch

import score_ref as R
from flowtron_amd import align, ops, score

pytestmark = pytest.mark.gpu

FPW = 4                    # frames of a workgroup of frame_ll_k (csrc/score.hip: LL_FPW)


def ll_case(T, M, n_ls, seed, fill):
    """B = 4 utterances of lengths (T, 1, a middle value, T - 1); log_s as column slices of [T, B, 2M] tensors (row stride 2M);
    `fill` behind the lengths and in the other half of the wide tensors -> (z, wide tensors, lengths) on the host"""
    rs = np.random.RandomState(seed)
    lens = [T, 1, max(T // 2, 1), max(T - 1, 1)]
    z = rs.standard_normal((T, 4, M)).astype(np.float32)
    wides = []
    for _ in range(n_ls):
        w = np.full((T, 4, 2 * M), fill, np.float32)
        w[:, :, M:] = 0.3 * rs.standard_normal((T, 4, M)).astype(np.float32)
        wides.append(w)
    for b, n in enumerate(lens):
        z[n:, b] = fill
        for w in wides:
            w[n:, b] = fill
    return z, wides, lens


def run_ll(z, wides, lens, rev, sigma=1.0):
    M = z.shape[2]
    dev = [torch.from_numpy(w).cuda() for w in wides]
    views = [w[:, :, M:] for w in dev]                                      # row stride 2M
    assert all(v.stride(1) == 2 * M for v in views)
    got = score.frame_log_likelihood(torch.from_numpy(z).cuda(), views, lens, sigma, rev)
    assert got.frame_ll.dtype == torch.float64 and got.total.dtype == torch.float64 and got.frame_ll.is_cuda and got.total.is_cuda
    return got.frame_ll.cpu().numpy(), got.total.cpu().numpy()


@pytest.mark.parametrize("T", [1, 2, FPW - 1, FPW, FPW + 1, 257])
@pytest.mark.parametrize("M", [1, 3, 64, 65, 80, 128])
def test_likelihood_equals_the_float64_replay_alone_and_in_a_batch_and_reads_nothing_behind_the_lengths(M, T):
    for n_ls in (1, 2, 3):
        rev = [f % 2 == 1 for f in range(n_ls)]                             # alternating
        sigma = (1.0, 0.7, 1.3)[n_ls - 1]
        z, wides, lens = ll_case(T, M, n_ls, 1000 * M + 10 * T + n_ls, np.nan)
        fl, tot = run_ll(z, wides, lens, rev, sigma)
        rf, rt = R.frame_loglik(z, [w[:, :, M:] for w in wides], rev, lens, sigma)
        assert fl.tobytes() == rf.tobytes(), (n_ls, np.abs(fl - rf).max())
        assert tot.tobytes() == rt.tobytes(), (n_ls, tot, rt)
        assert np.isfinite(fl).all() and all(np.all(fl[b, n:] == 0.0) for b, n in enumerate(lens))
        # 1e30 where NaN was: nothing changes
        z2, wides2, _ = ll_case(T, M, n_ls, 1000 * M + 10 * T + n_ls, 1e30)
        fl2, tot2 = run_ll(z2, wides2, lens, rev, sigma)
        assert fl2.tobytes() == fl.tobytes() and tot2.tobytes() == tot.tobytes()
        # every utterance alone, cut to its own frames
        for b, n in enumerate(lens):
            one = run_ll(np.ascontiguousarray(z[:n, b:b + 1]), [np.ascontiguousarray(w[:n, b:b + 1]) for w in wides], [n], rev, sigma)
            assert one[0].tobytes() == fl[b:b + 1, :n].tobytes() and one[1].tobytes() == tot[b:b + 1].tobytes(), (n_ls, b)


def test_the_reversed_flag_moves_frames_and_leaves_the_total():
    """z and flow 0's log_s are the same in every frame of an utterance, flow 1's log_s is a ramp in time: swapping flow 1's flag
    must hand back every utterance's frame_ll flipped over its OWN length, bit for bit.  The lengths are powers of two <= 256:
    there the documented total (partial sums p_i = ll[i], tree p_i + p_{i+h}) pairs the same frames under the flip, each pair
    in the other order, and addition commutes -- so the totals must be equal bit for bit as well."""
    T, B, M = 8, 4, 80
    lens = [8, 4, 2, 1]
    rs = np.random.RandomState(5)
    z = np.repeat(rs.standard_normal((1, B, M)).astype(np.float32), T, 0)
    w0 = np.repeat(0.3 * rs.standard_normal((1, B, 2 * M)).astype(np.float32), T, 0)
    w1 = np.zeros((T, B, 2 * M), np.float32)
    w1[:, :, M:] = (np.arange(T, dtype=np.float32)[:, None, None] ** 2) * 0.125 * (np.arange(M) % 3)[None, None, :]
    a, ta = run_ll(z, [w0, w1], lens, [False, False])
    b_, tb = run_ll(z, [w0, w1], lens, [False, True])
    for b, n in enumerate(lens):
        assert b_[b, :n].tobytes() == a[b, :n][::-1].tobytes(), b
        assert n == 1 or not np.array_equal(a[b, :n], b_[b, :n])
    assert ta.tobytes() == tb.tobytes()
    assert a.tobytes() == R.frame_loglik(z, [w0[:, :, M:], w1[:, :, M:]], [False, False], lens)[0].tobytes()


def attn_rows(kind, T, L, seed):
    rs = np.random.RandomState(seed)
    if kind == "softmax":
        s = torch.from_numpy(rs.standard_normal((T, L)).astype(np.float32))
        return torch.softmax(s, 1).numpy()
    return (rs.randint(0, 17, size=(T, L)) / 8.0).astype(np.float32)       # multiples of 1/8 in [0, 2]: ties everywhere


def check_diag(d, host_view, il, ol, dev_view=None):
    """d: attention_diagnostics of the device view, host_view: the same [F, B, T, L] view on the host"""
    rp, rc, rf = R.attn_diagnostics(host_view, il, ol)
    if dev_view is not None:                                               # the kernel's own focus_sum, bit for bit
        i32, o32 = torch.tensor(il, dtype=torch.int32).cuda(), torch.tensor(ol, dtype=torch.int32).cuda()
        assert ops.attn_diagnostics(dev_view, i32, o32)[2].cpu().numpy().tobytes() == rf.tobytes()
    if d.peaks.dim() == 2:                                                 # a [B, T, L] input: the fields come without the flow dimension
        d = score.AttentionDiagnostics(*[x[None] for x in d])
    assert d.peaks.dtype == torch.int32 and d.peaks.is_cuda and d.focus.dtype == torch.float64 and d.coverage.dtype == torch.float64
    assert np.array_equal(d.peaks.cpu().numpy(), rp)
    for k, name in enumerate(R.COUNTERS):
        got = getattr(d, name)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), rc[:, :, k]), name
    n, l = np.array(ol, np.float64), np.array(il, np.float64)
    # focus_sum bit for bit: every pmax is 0 or >= 2^-8 with a last bit >= 2^-32 and at most 2^11 of them sum below 2^12, so the
    # float64 sum is exact in any order; focus = focus_sum / n is one correctly rounded division on either side
    assert (rf / n[None, :]).tobytes() == d.focus.cpu().numpy().tobytes()
    assert np.array_equal(d.coverage.cpu().numpy(), rc[:, :, 0] / l[None, :])


@pytest.mark.parametrize("T", [1, 2, 70])
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 130])
def test_diagnostics_equal_the_replay_on_a_ragged_batch_inside_a_padded_view(L, T):
    lens = [(T, L), (1, 1), (max(T // 2, 1), max(L // 2, 1)), (T, 1), (max(T - 1, 1), L)]     # (n, l)
    il, ol = [l for _, l in lens], [n for n, _ in lens]
    for F in (1, 2):
        for kind in ("softmax", "grid"):
            big = torch.full((F + 1, 7, T + 5, L + 6), float("nan"))
            view = big[1:, 1:6, 2:2 + T, 3:3 + L]                           # [F, 5, T, L]
            for f in range(F):
                for b, (n, l) in enumerate(lens):
                    view[f, b, :n, :l] = torch.from_numpy(attn_rows(kind, n, l, 7 * L + T + 10 * f + b))
            dev = big.cuda()
            v = dev[1:, 1:6, 2:2 + T, 3:3 + L]
            assert not v.is_contiguous()
            d = score.attention_diagnostics(v, il, torch.tensor(ol).cuda())  # lengths on the host and on the device
            check_diag(d, view.numpy(), il, ol, v)
            dev[torch.isnan(dev)] = 1e30
            again = score.attention_diagnostics(v, il, ol)
            for x, y in zip(d, again):
                assert torch.equal(x, y)
    one = score.attention_diagnostics(v[0], il, ol)                          # [B, T, L]: the same fields without the flow dimension
    for x, y in zip(one, again):
        assert torch.equal(x, y[0])


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 130])
def test_hard_staircases_give_their_counters_exactly(L):
    rs = np.random.RandomState(L)
    il = [L, max(L // 2, 1), 1]
    d = np.zeros((3, L), np.int32)
    for b, l in enumerate(il):
        d[b, :l] = rs.randint(1, 5, size=l)
    rows = align.durations_to_alignment(torch.from_numpy(d).cuda(), il)     # [3, N, L] one-hot, natural time
    ol = [int(x) for x in d.sum(1)]
    diag = score.attention_diagnostics(rows, il, ol)
    check_diag(diag, rows.cpu().numpy()[None], il, ol, rows[None])
    assert diag.n_backward.tolist() == [0, 0, 0] and diag.n_skipped.tolist() == [0, 0, 0]
    assert diag.coverage.tolist() == [1.0, 1.0, 1.0] and diag.n_attended.tolist() == il
    assert diag.longest_run.tolist() == [int(d[b].max()) for b in range(3)]
    assert diag.first_peak.tolist() == [0, 0, 0] and diag.last_peak.tolist() == [l - 1 for l in il]
    assert diag.focus.tolist() == [1.0, 1.0, 1.0]
    assert score.healthy(diag, il).tolist() == [True, True, True]
    assert score.healthy(diag, il, max_run=int(d.max()) - 1).tolist() == [bool(d[b].max() < d.max()) for b in range(3)]


def test_runs_that_cross_the_scan_tiles_of_1024_frames():
    """more frames than the workgroup has threads: the run lengths carry from one tile of the scan into the next"""
    d = np.array([[1027, 3, 0], [5, 1030, 2], [1024, 1, 1025]], np.int32)
    il = [2, 3, 3]
    rows = align.durations_to_alignment(torch.from_numpy(d).cuda(), il)
    ol = [int(x) for x in d.sum(1)]
    assert rows.shape[1] == 2050
    diag = score.attention_diagnostics(rows, il, ol)
    check_diag(diag, rows.cpu().numpy()[None], il, ol, rows[None])
    assert diag.longest_run.tolist() == [1027, 1030, 1025]
    back = torch.flip(rows[2:3, :2050], (1,))                                # the same run structure walked backwards
    diag = score.attention_diagnostics(back, [3], [2050])
    check_diag(diag, back.cpu().numpy()[None], [3], [2050], back[None])
    assert diag.n_backward.tolist() == [2] and diag.longest_run.tolist() == [1025] and diag.n_attended.tolist() == [3]
    assert score.healthy(diag, [3]).tolist() == [False]


@pytest.fixture(scope="module")
def case():
    """the small 2-flow test model with the non-zero coupling weights oracle.synth makes for the goldens, fp32 operand mode, a
    ragged batch of three handed over in an order that is NOT sorted by text length (the fixture of tests/test_gpu_align.py)"""
    import flowtron
    from oracle import synth
    old = os.environ.get("FLOWTRON_MFMA")
    os.environ["FLOWTRON_MFMA"] = "f32"
    cfg = dict(synth.SMALL_MODEL_CONFIG)
    sd = synth.make_state_dict(cfg, seed=31)
    m = flowtron.Flowtron(**cfg)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    sorted_b = synth.make_batch(cfg, [30, 17, 21], [9, 7, 5], seed=31, with_prior=False)       # sorted by text length
    order = [2, 0, 1]                                                      # the caller's utterance i = sorted utterance order[i]
    idx = torch.tensor(order)
    b = {k: sorted_b[k][idx].cuda() for k in ("mel", "speaker_ids", "text", "in_lens", "out_lens")}
    with torch.no_grad():
        out = m(*[sorted_b[k].cuda() for k in ("mel", "speaker_ids", "text", "in_lens", "out_lens")], None)
    yield dict(cfg=cfg, sd=sd, m=m, sorted=sorted_b, order=order, b=b, il=b["in_lens"].tolist(), ol=b["out_lens"].tolist(), out=out)
    if old is None:
        os.environ.pop("FLOWTRON_MFMA", None)
    else:
        os.environ["FLOWTRON_MFMA"] = old


def staircase(N, L):
    """an asymmetric staircase [N, L]: token j holds j + 1 frames (the last one what is left)"""
    peaks = np.minimum(np.repeat(np.arange(L), np.arange(1, L + 1))[:N], L - 1)
    assert len(peaks) == N and not np.array_equal(peaks, (L - 1 - peaks)[::-1])
    a = np.zeros((N, L), np.float32)
    a[np.arange(N), peaks] = 1.0
    return torch.from_numpy(a)


def test_infer_attention_maps_puts_forced_rows_back_in_flow_order_and_natural_time(case):
    m, sb = case["m"], case["sorted"]
    N, Lt, M = 15, 5, sb["mel"].shape[1]
    S = staircase(N, Lt).cuda()
    g = torch.Generator().manual_seed(3)
    residual = (0.5 * torch.randn(1, M, N, generator=g)).cuda()
    # flows order, each in its flow's own time order: flow 1 decodes the utterance backwards
    forced = [S, torch.flip(S, (0,))]
    mel, aws, lengths = m.infer(residual, sb["speaker_ids"][:1].cuda(), sb["text"][:1, :Lt].cuda(), gate_threshold=1.0, attns=forced,
                                return_lengths=True)
    assert lengths.tolist() == [N] and len(aws) == 2
    maps = score.infer_attention_maps(aws, lengths)
    assert tuple(maps.shape) == (2, 1, N, Lt) and maps.is_cuda and maps.dtype == torch.float32
    for f in range(2):
        assert torch.equal(maps[f, 0], S), f
    diag = score.attention_diagnostics(maps, [Lt], lengths)
    assert score.healthy(diag, [Lt]).tolist() == [[True], [True]]
    assert diag.longest_run.tolist() == [[Lt], [Lt]]


def test_infer_attention_maps_of_a_batch_equal_each_utterance_decoded_alone(case):
    m, sb = case["m"], case["sorted"]
    M, Lt = sb["mel"].shape[1], 9
    il, ol = [9, 6], [5, 8]
    g = torch.Generator().manual_seed(4)
    residual = (0.5 * torch.randn(2, M, 8, generator=g)).cuda()
    sid, text = sb["speaker_ids"][:2].cuda(), sb["text"][:2, :Lt].cuda()
    mel, aws, lengths = m.infer(residual, sid, text, gate_threshold=1.0, in_lens=il, out_lens=ol, return_lengths=True)
    assert lengths.tolist() == ol
    maps = score.infer_attention_maps(aws, lengths)
    assert tuple(maps.shape) == (2, 2, 8, Lt)
    for b in range(2):
        _, aw1, n1 = m.infer(residual[b:b + 1, :, :ol[b]], sid[b:b + 1], text[b:b + 1, :il[b]], gate_threshold=1.0, return_lengths=True)
        alone = score.infer_attention_maps(aw1, n1)                         # [2, 1, n, l]
        assert torch.equal(maps[:, b, :ol[b], :il[b]], alone[:, 0]), b
        assert float(maps[:, b, ol[b]:].abs().sum()) == 0.0 and float(maps[:, b, :, il[b]:].abs().sum()) == 0.0
        assert float(alone.sum()) > 0.0


def test_log_likelihood_equals_the_kernel_on_a_direct_sorted_forward(case):
    m, b, order, out, sb = case["m"], case["b"], case["order"], case["out"], case["sorted"]
    assert case["il"] != sorted(case["il"], reverse=True)
    got = m.log_likelihood(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
    B, M, T = b["mel"].shape
    assert tuple(got.frame_ll.shape) == (B, T) and tuple(got.total.shape) == (B,) and tuple(got.nll_per_dim.shape) == (B,)
    assert all(x.dtype == torch.float64 and x.is_cuda for x in got)
    assert [hasattr(f, "ar_step") for f in m.flows] == [False, True]
    direct = score.frame_log_likelihood(out[0], out[1], sb["out_lens"].tolist(), 1.0, [False, True])
    idx = torch.tensor(order).cuda()
    assert torch.equal(got.frame_ll, direct.frame_ll[idx]) and torch.equal(got.total, direct.total[idx])
    # and the replay on the forward's own tensors
    rf, rt = R.frame_loglik(out[0].cpu().numpy(), [x.cpu().numpy() for x in out[1]], [False, True], sb["out_lens"].tolist())
    assert direct.frame_ll.cpu().numpy().tobytes() == rf.tobytes() and direct.total.cpu().numpy().tobytes() == rt.tobytes()
    # lists, and lengths on the host, give the same
    again = m.log_likelihood(b["mel"], b["speaker_ids"], b["text"], case["il"], b["out_lens"].cpu())
    assert all(torch.equal(x, y) for x, y in zip(got, again))


def test_frame_weighted_mean_of_nll_per_dim_is_the_loss(case):
    """bound: the worst case of an fp32 sum of N = n M (F + 1) terms in any order, N 2^-24 sum|terms|, over the loss's n M;
    sum|terms| from the float64 tensors of the same forward"""
    import flowtron
    m, b, out, sb, order = case["m"], case["b"], case["out"], case["sorted"], case["order"]
    got = m.log_likelihood(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
    crit = flowtron.FlowtronLoss(1.0, False, True, False)
    with torch.no_grad():
        nll = crit(out, sb["gate_target"].cuda(), sb["in_lens"].cuda(), sb["out_lens"].cuda())[0]
    ol = np.array(case["ol"], np.float64)
    mean = float((got.nll_per_dim.cpu().numpy() * ol).sum() / ol.sum())
    M, F = b["mel"].shape[1], len(m.flows)
    z, ls = out[0].double().cpu().numpy(), [x.double().cpu().numpy() for x in out[1]]
    terms = 0.0
    for pos, n in enumerate(sb["out_lens"].tolist()):
        terms += np.abs(z[:n, pos] ** 2 / 2.0).sum() + sum(np.abs(x[:n, pos]).sum() for x in ls)
    n_all = ol.sum()
    bound = n_all * M * (F + 1) * 2.0 ** -24 * terms / (n_all * M)
    print("nll: loss %.9g, frame-weighted mean of nll_per_dim %.9g, deviation %.3e, bound %.3e" % (nll.item(), mean, abs(nll.item() - mean), bound))
    assert abs(nll.item() - mean) <= bound


def _oracle_nll(o, pos, n, M, sigma=1.0):
    z = o[0][:n, pos].double().numpy()
    return float(((z ** 2).sum() / (2 * sigma * sigma) - sum(x[:n, pos].double().numpy().sum() for x in o[1])) / (n * M))


def _margin(o, pos, n, M, F, tol=1e-4):
    """the forward-parity test of tests/test_gpu_model.py grants z and log_s 1e-4 against the reference in fp32 mode; through
    (sum z^2 / 2 - sum log_s) / (n M) that is sum(|z| tol + tol^2 / 2) + F n M tol, over n M"""
    z = np.abs(o[0][:n, pos].double().numpy())
    return float(((z * tol + tol * tol / 2).sum() + F * n * M * tol) / (n * M))


def test_per_utterance_nll_against_the_cpu_oracle(case):
    """Per-utterance NLL per dimension, formed in float64 from the oracle's z and log_s, against Flowtron.log_likelihood's.
    Measured on an MI355X: deviations 2.634e-07, 2.145e-08, 2.784e-08 for the utterances of 21, 30 and 17 frames, against
    margins of 7.479e-04, 5.973e-04, 6.905e-04."""
    from oracle import flowtron_oracle as O
    m, b, sb, order, cfg, sd = case["m"], case["b"], case["sorted"], case["order"], case["cfg"], case["sd"]
    got = m.log_likelihood(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"]).nll_per_dim.cpu().numpy()
    with torch.no_grad():
        o = O.forward(sd, cfg, sb["mel"], sb["speaker_ids"], sb["text"], sb["in_lens"], sb["out_lens"], None)
    M, F = b["mel"].shape[1], len(m.flows)
    for i, pos in enumerate(order):
        n = case["ol"][i]
        want, margin = _oracle_nll(o, pos, n, M), _margin(o, pos, n, M, F)
        print("utterance %d (%d frames): nll per dim %.9g, oracle %.9g, deviation %.3e, margin %.3e" % (i, n, got[i], want, abs(got[i] - want), margin))
        assert abs(got[i] - want) <= margin, i


def test_use_cases_end_to_end(case):
    from oracle import flowtron_oracle as O
    m, b, sb, cfg, sd = case["m"], case["b"], case["sorted"], case["cfg"], case["sd"]
    il, ol = case["il"], case["ol"]
    # corpus cleaning: alignments -> diagnostics -> healthy
    z, attn, logp = m.alignments(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
    diag = score.attention_diagnostics(attn, il, ol)
    F, B, T = len(m.flows), len(il), b["mel"].shape[2]
    assert tuple(diag.peaks.shape) == (F, B, T) and all(tuple(x.shape) == (F, B) for x in diag[1:])
    ok = score.healthy(diag, il)
    loose = score.healthy(diag, il, max_backward=T, max_skipped=T * 9, min_coverage=0.0, require_end=False)
    assert ok.dtype == torch.bool and ok.is_cuda and tuple(ok.shape) == (F, B) and bool(loose.all())
    print("coverage", diag.coverage.tolist(), "backward", diag.n_backward.tolist(), "skipped", diag.n_skipped.tolist(),
          "healthy", ok.tolist())
    # a damaged utterance: the mel of sorted utterance 0 with the text of utterance 1
    mel = torch.stack([sb["mel"][0], sb["mel"][0]])
    text = torch.stack([sb["text"][0], sb["text"][1]])
    sid = torch.stack([sb["speaker_ids"][0], sb["speaker_ids"][0]])
    i2, o2 = [int(sb["in_lens"][0]), int(sb["in_lens"][1])], [int(sb["out_lens"][0])] * 2
    got = m.log_likelihood(mel.cuda(), sid.cuda(), text.cuda(), i2, o2)
    per_frame = (got.total.cpu().numpy() / np.array(o2, np.float64)).tolist()
    with torch.no_grad():
        o = O.forward(sd, cfg, mel, sid, text, torch.tensor(i2), torch.tensor(o2), None)
    M = mel.shape[1]
    ref = [-_oracle_nll(o, pos, o2[pos], M) * M for pos in range(2)]       # per frame, without the Gaussian constant
    margin = sum(_margin(o, pos, o2[pos], M, F) * M for pos in range(2))
    print("log-likelihood per frame: intact %.6f, damaged %.6f (oracle, without the constant: %.6f, %.6f)" % (per_frame[0], per_frame[1], ref[0], ref[1]))
    if ref[0] - ref[1] > margin:                                           # only where the untrained model separates them at all
        assert per_frame[0] > per_frame[1]
