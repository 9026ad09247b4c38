"""Token durations and pace control on the device (-m gpu): the search kernel against its float32 replay (tests/align_ref.py)
bit for bit, the expansion kernel against a numpy one-hot expansion, Flowtron.alignments against the batched forward's own
maps, Flowtron.infer_aligned against infer(attns=) one utterance at a time, and the round trip mel -> z, attention -> mel."""
import os

import numpy as np
import pytest
import torch

import align_ref as R
from flowtron_amd import align

pytestmark = pytest.mark.gpu

# (T, L): edges; the wave boundary; the 256-thread boundary; the limit
SHAPES = [(1, 1), (5, 1), (4, 4), (9, 2), (70, 63), (70, 64), (70, 65), (300, 255), (300, 256), (300, 257), (1030, 1024)]


def scores(kind, T, L, seed):
    rs = np.random.RandomState(seed)
    if kind == "normal":
        return rs.standard_normal((T, L)).astype(np.float32)
    return (-rs.randint(0, 17, size=(T, L)) / 8.0).astype(np.float32)       # multiples of 1/8 in [-2, 0]: ties everywhere


def search(s, in_lens, out_lens):
    """-> numpy (path, durations, score) of monotonic_alignment on device scores s"""
    path, dur, score = align.monotonic_alignment(s, in_lens, out_lens, return_score=True)
    assert path.dtype == torch.int32 and dur.dtype == torch.int32 and score.dtype == torch.float32
    assert path.is_cuda and dur.is_cuda and score.is_cuda
    return path.cpu().numpy(), dur.cpu().numpy(), score.cpu().numpy()


def assert_equals_replay(got, s, b=0):
    """utterance b of `got` against the float32 replay of s [T_b, L_b]: the same bits"""
    path, dur, score = got
    T, L = s.shape
    rp, rd, rq = R.replay(s, np.float32)
    assert np.array_equal(path[b, :T], rp), (b, T, L)
    assert np.all(path[b, T:] == -1)
    assert np.array_equal(dur[b, :L], rd), (b, T, L)
    assert np.all(dur[b, L:] == 0)
    assert score[b:b + 1].tobytes() == np.float32(rq).tobytes() or (np.isnan(score[b]) and np.isnan(rq)), (b, score[b], rq)


@pytest.mark.parametrize("kind", ["normal", "grid"])
@pytest.mark.parametrize("T,L", SHAPES)
def test_search_equals_the_float32_replay_bit_for_bit(T, L, kind):
    s = scores(kind, T, L, 100 * T + L)
    got = search(torch.from_numpy(s)[None].cuda(), [L], [T])
    assert_equals_replay(got, s)
    assert got[1].sum() == T and got[1].min() >= 1


def test_ragged_batch_inside_a_padded_view_never_reads_behind_the_lengths():
    """six utterances of one call, their scores inside a non-contiguous [F, B, T, L] view; everything behind the lengths and
    around the view is NaN, then 1e30: nothing of it may be read"""
    lens = [(75, 70), (40, 40), (9, 1), (75, 3), (64, 64), (12, 5)]         # (T_b, L_b)
    big = torch.full((2, 8, 80, 80), float("nan"))
    view = big[1, 1:7, 2:77, 3:73]                                         # [6, 75, 70]
    ss = []
    for b, (T, L) in enumerate(lens):
        s = scores("grid" if b % 2 else "normal", T, L, 50 + b)
        view[b, :T, :L] = torch.from_numpy(s)
        ss.append(s)
    dev = big.cuda()
    v = dev[1, 1:7, 2:77, 3:73]
    assert not v.is_contiguous()
    il, ol = [L for _, L in lens], [T for T, _ in lens]
    got = search(v, torch.tensor(il), torch.tensor(ol).cuda())             # lengths on the host and on the device
    for b, s in enumerate(ss):
        assert_equals_replay(got, s, b)
    sentinel = torch.isnan(dev)
    dev[sentinel] = 1e30
    again = search(v, il, ol)
    for a, b_ in zip(got, again):
        assert a.tobytes() == b_.tobytes()


def test_equal_scores_a_band_and_minus_infinity_everywhere():
    T, L = 90, 70
    flat = np.zeros((T, L), np.float32)                                    # every path ties: the earliest advancing one
    got = search(torch.from_numpy(flat)[None].cuda(), [L], [T])
    assert_equals_replay(got, flat)
    assert np.array_equal(got[0][0], np.minimum(np.arange(T), L - 1))
    band = scores("normal", T, L, 8)
    t, l = np.meshgrid(np.arange(T), np.arange(L), indexing="ij")
    band[np.abs(t * (L - 1) / (T - 1) - l) > 6] = -np.inf                  # only a diagonal band is allowed
    got = search(torch.from_numpy(band)[None].cuda(), [L], [T])
    assert_equals_replay(got, band)
    assert np.isfinite(got[2][0])
    assert np.all(np.isfinite(band[np.arange(T), got[0][0]]))              # the path stays inside the band
    ninf = np.full((T, L), -np.inf, np.float32)
    got = search(torch.from_numpy(ninf)[None].cuda(), [L], [T])
    assert_equals_replay(got, ninf)
    assert got[2][0] == -np.inf and got[0][0, 0] == 0 and got[0][0, -1] == L - 1
    assert set(np.diff(got[0][0]).tolist()) <= {0, 1} and got[1][0].min() >= 1 and got[1][0].sum() == T


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("L", [63, 64, 65, 1024])
def test_expansion_equals_the_numpy_one_hot_rows(L, reverse):
    """zero and negative durations, ragged in_lens, N larger than every total and N that cuts the longest utterance"""
    rs = np.random.RandomState(L)
    B = 4
    d = rs.randint(-1, 4, size=(B, L)).astype(np.int32)
    d[1] = 0                                                               # an utterance of no frames at all
    d[2, :5] = [40, 0, 0, 33, 1]                                           # tokens longer than a workgroup's rows
    il = [L, L, max(L // 2, 1), 1]
    totals = [int(np.maximum(d[b, :il[b]], 0).sum()) for b in range(B)]
    dd = torch.from_numpy(d).cuda()
    for N in (None, max(totals) + 37, max(totals) // 2):
        rows = align.durations_to_alignment(dd, il, n_frames=N, reverse=reverse)
        n = max(totals) if N is None else N
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (B, n, L)
        got = rows.cpu().numpy()
        for b in range(B):
            assert np.array_equal(got[b], R.one_hot_rows(d[b], il[b], n, reverse)), (b, N)


@pytest.fixture(scope="module")
def case():
    """synth.SMALL_MODEL_CONFIG with the coupling weights oracle.synth makes for the goldens (non-zero: a freshly constructed
    model's flows are the identity), fp32 operand mode, a ragged batch of three handed over in an order that is NOT sorted by
    text length"""
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
    yield dict(cfg=cfg, sd=sd, m=m, sorted=sorted_b, order=order, b=b, il=b["in_lens"].tolist(), ol=b["out_lens"].tolist())
    if old is None:
        os.environ.pop("FLOWTRON_MFMA", None)
    else:
        os.environ["FLOWTRON_MFMA"] = old


def test_alignments_equal_the_forwards_own_maps_in_natural_time(case):
    m, b, sb, order = case["m"], case["b"], case["sorted"], case["order"]
    il, ol = case["il"], case["ol"]
    assert il != sorted(il, reverse=True)
    z, attn, logp = m.alignments(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
    B, M, T = b["mel"].shape
    F, Lt = len(m.flows), b["text"].shape[1]
    assert tuple(z.shape) == (B, M, T) and tuple(attn.shape) == (F, B, T, Lt) and tuple(logp.shape) == (F, B, T, Lt)
    assert F >= 2                                                          # an odd flow is among them
    with torch.no_grad():
        out = m(sb["mel"].cuda(), sb["speaker_ids"].cuda(), sb["text"].cuda(), sb["in_lens"].cuda(), sb["out_lens"].cuda(), None)
    for got, ref in ((attn, out[3]), (logp, out[4])):
        for f in range(F):
            want = torch.zeros(B, T, Lt)
            for i, pos in enumerate(order):
                r = ref[f][pos, :ol[i], :il[i]].cpu()
                want[i, :ol[i], :il[i]] = torch.flip(r, (0,)) if f % 2 == 1 else r       # odd flows: reversed by length
            assert torch.equal(got[f].cpu(), want), f
    assert torch.equal(z, m.latents(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"]))
    with pytest.raises(ValueError, match="eval"):
        m.train()
        try:
            m.alignments(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
        finally:
            m.eval()


def _hard_rows(case, seed):
    """durations of at least one frame per token for the case's three utterances -> (durations on the device, totals)"""
    rs = np.random.RandomState(seed)
    Lt = case["b"]["text"].shape[1]
    d = np.zeros((3, Lt), np.int32)
    for i, l in enumerate(case["il"]):
        d[i, :l] = rs.randint(1, 5, size=l)
    return torch.from_numpy(d).cuda(), [int(x) for x in d.sum(1)]


def test_infer_aligned_equals_infer_with_forced_rows_one_utterance_at_a_time(case):
    m, b, il = case["m"], case["b"], case["il"]
    d, totals = _hard_rows(case, 4)
    assert len(set(totals)) == 3
    rows = align.durations_to_alignment(d, il)                             # [B, N, L] natural time
    back = align.durations_to_alignment(d, il, reverse=True)               # each utterance's own frames reversed
    N, M = rows.shape[1], b["mel"].shape[1]
    assert N == max(totals)
    g = torch.Generator().manual_seed(9)
    residual = (0.5 * torch.randn(3, M, N, generator=g)).cuda()
    mel, lengths = m.infer_aligned(residual, b["speaker_ids"], b["text"], rows, in_lens=il, n_frames=totals)
    assert lengths.dtype == torch.int64 and not lengths.is_cuda and lengths.tolist() == totals
    assert tuple(mel.shape) == (3, M, N)
    per_flow = torch.stack([rows] * len(m.flows))
    mel4, lengths4 = m.infer_aligned(residual, b["speaker_ids"], b["text"], per_flow, in_lens=il, n_frames=totals)
    assert torch.equal(mel4, mel) and lengths4.tolist() == totals
    for i in range(3):
        n, l = totals[i], il[i]
        forced = [(back if f % 2 == 1 else rows)[i, :n, :l] for f in range(len(m.flows))]
        assert torch.equal(forced[1], torch.flip(rows[i, :n, :l], (0,)))
        one, _ = m.infer(residual[i:i + 1, :, :n], b["speaker_ids"][i:i + 1], b["text"][i:i + 1, :l], attns=forced, gate_threshold=1.0)
        assert tuple(one.shape) == (1, M, n)
        assert torch.equal(mel[i, :, :n], one[0]), i
        assert float(mel[i, :, n:].abs().sum()) == 0.0
    with pytest.raises(ValueError, match="forced alignments"):             # infer itself still takes them one at a time
        m.infer(residual, b["speaker_ids"], b["text"], attns=[rows, rows])
    with pytest.raises(ValueError, match="alignment must be"):
        m.infer_aligned(residual, b["speaker_ids"], b["text"], rows[:, :-1], in_lens=il)


def test_round_trip_mel_to_latents_and_attention_and_back(case):
    """mel -> alignments -> infer_aligned(z, the per-flow soft attention) gives mel back.  Bound: what the CPU oracle's own
    forward followed by its forced infer deviates on the same case, plus the 1e-4 that test_infer_vs_reference_golden grants the
    decode kernels against the reference in fp32.
    Measured on an MI355X: the oracle's round trip deviates 1.431e-06, the device's 1.907e-06."""
    from oracle import flowtron_oracle as O
    m, b, sb, order, cfg, sd = case["m"], case["b"], case["sorted"], case["order"], case["cfg"], case["sd"]
    il, ol = case["il"], case["ol"]
    z, attn, _ = m.alignments(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
    assert float((z - b["mel"]).abs().max()) > 1e-2                        # the flows are not the identity
    mel, lengths = m.infer_aligned(z, b["speaker_ids"], b["text"], attn, in_lens=il, n_frames=ol)
    assert lengths.tolist() == ol
    # the oracle's own round trip: batched forward, then every utterance alone along its attention, in each flow's own order
    with torch.no_grad():
        o = O.forward(sd, cfg, sb["mel"], sb["speaker_ids"], sb["text"], sb["in_lens"], sb["out_lens"], None)
        dev_o = dev_d = 0.0
        for i, pos in enumerate(order):
            n, l = ol[i], il[i]
            forced = [a[pos, :n, :l] for a in o[3]]
            back, _ = O.infer(sd, cfg, o[0][:n, pos].t()[None], sb["speaker_ids"][pos:pos + 1], sb["text"][pos:pos + 1, :l],
                              gate_threshold=1.0, attns=forced)
            assert back.shape[2] == n
            dev_o = max(dev_o, float((back[0] - sb["mel"][pos, :, :n]).abs().max()))
            dev_d = max(dev_d, float((mel[i, :, :n].cpu() - sb["mel"][pos, :, :n]).abs().max()))
            assert float(mel[i, :, n:].abs().sum()) == 0.0
    print("round trip: oracle deviation %.3e, device deviation %.3e" % (dev_o, dev_d))
    assert dev_d <= dev_o + 1e-4, (dev_d, dev_o)


@pytest.mark.parametrize("pace", [0.5, 2.0])
def test_pace_sets_the_frames_of_every_utterance(case, pace):
    m, b, il, ol = case["m"], case["b"], case["il"], case["ol"]
    z, attn, logp = m.alignments(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
    path, dur = align.monotonic_alignment(logp[0], il, ol)
    assert dur.sum(1).tolist() == ol
    scaled, totals = align.scale_durations(dur, il, pace)
    assert scaled.is_cuda
    for i, l in enumerate(il):                                             # round(T / pace), or what one frame per token forces
        r = [0] + [int(np.floor(e / pace + 0.5)) for e in np.cumsum(dur[i, :l].cpu().numpy())]
        assert int(totals[i]) == max(r[j + 1] + (l - 1 - j) for j in range(-1, l))
        assert int(totals[i]) >= int(np.floor(ol[i] / pace + 0.5))
    rows = align.durations_to_alignment(scaled, il)
    N = int(totals.max())
    assert rows.shape[1] == N
    g = torch.Generator().manual_seed(int(pace * 10))
    residual = (0.5 * torch.randn(3, b["mel"].shape[1], N, generator=g)).cuda()
    mel, lengths = m.infer_aligned(residual, b["speaker_ids"], b["text"], rows, in_lens=il, n_frames=totals)
    assert torch.equal(lengths, totals) and mel.shape[2] == N
    for i in range(3):
        n = int(totals[i])
        assert torch.isfinite(mel[i]).all()
        assert float(mel[i, :, n:].abs().sum()) == 0.0
