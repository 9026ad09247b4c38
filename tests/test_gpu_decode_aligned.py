"""Decode along given alignments in the persistent launches (-m gpu): Flowtron.infer_aligned(persistent=True),
AR_Step.infer_batch(forced=), ft_decode_flow_batch_forced (csrc/decode_forced.hip: dec_persist_batch_k<F32, true>).
Full-width synthetic 2-flow models (the launch geometry is fixed at H 1024), fp32 weights and bf16 weight images.

  1. the grouping is invisible: every utterance of a batch is bit for bit what it is when decoded alone
  2. every flow against tests/decode_ref64.py on the launch's own V, residual and rows, within decode_ref64.tolerance =
     10 x the fp32 oracle's own deviation (the bound of tests/test_gpu_decode_f64.py; nothing new); the written attention
     rows equal the given rows exactly
  3. a free-running decode's own attention, fed back, reproduces that decode
  4. which kernel ran: stage stamps, failure counter, status word, calls of the entries
  5. the round trip mel -> z, attention -> mel of tests/test_gpu_align.py with persistent=True
  6. routing outside the geometry and with the switches off
A launch that does not complete is decoded again on the staged chain by AR_Step.infer_batch (model.py, behind
check_persist_status); no test provokes that."""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import decode_ref64 as R
import test_gpu_decode_batch as TB
import test_gpu_decode_f64 as T64
from flowtron_amd import align

pytestmark = pytest.mark.gpu

MODES = ["f32", "bf16"]
IN_LENS = [13, 7, 13, 10, 7]             # three different text lengths
N_FRAMES = [29, 16, 31, 25, 18]          # what RandomState(1) draws below: five different frame counts, 12 .. 40


def hard_case(per_flow):
    """B = 5 utterances: durations of 1 .. 4 frames per token (as test_gpu_align._hard_rows makes them) -> (residual, spk, text,
    alignment [B,N,L] or, per_flow, [F,B,N,L] with the durations of flow 1 permuted among each utterance's tokens)"""
    rs = np.random.RandomState(1)
    Lt = max(IN_LENS)
    d = np.zeros((2, 5, Lt), np.int32)
    for b, l in enumerate(IN_LENS):
        d[0, b, :l] = rs.randint(1, 5, size=l)
    for b, l in enumerate(IN_LENS):
        d[1, b, :l] = d[0, b, :l][rs.permutation(l)]
    assert [int(x) for x in d[0].sum(1)] == N_FRAMES == [int(x) for x in d[1].sum(1)]
    rows = [align.durations_to_alignment(torch.from_numpy(d[f]).cuda(), IN_LENS) for f in range(2)]
    assert tuple(rows[0].shape) == (5, max(N_FRAMES), Lt)
    residual, spk, text = TB.inputs(5, max(N_FRAMES), Lt, seed=21, n_speakers=1)
    if per_flow:
        assert not torch.equal(rows[0], rows[1])
        return residual, spk, text, torch.stack(rows)
    return residual, spk, text, rows[0]


def aligned(m, mode, residual, spk, text, alignment, il, nf, idx=None, **kw):
    """infer_aligned of the utterances idx (None = all) of the case"""
    if idx is not None:
        residual, spk, text = residual[idx], spk[idx], text[idx]
        alignment = alignment[:, idx] if alignment.dim() == 4 else alignment[idx]
        il, nf = [il[b] for b in idx], [nf[b] for b in idx]
    with TB.env(FLOWTRON_MFMA=mode):
        return m.infer_aligned(residual, spk, text, alignment, in_lens=il, n_frames=nf, **kw)


def count_calls(monkeypatch):
    """calls of the decode entries, as test_gpu_decode_batch.count_calls counts them"""
    from flowtron_amd import _lib as L
    lib = L.lib()
    calls = {}
    for name in ("ft_decode_flow", "ft_decode_flow_batch", "ft_decode_flow_batch_keys", "ft_decode_flow_batch_forced"):
        fn = getattr(lib, name)
        calls[name] = 0

        def shim(*a, _fn=fn, _k=name):
            calls[_k] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, shim)
    return calls


def need_persist():
    if not T64.persistent_available():
        pytest.skip("persistent kernels not usable on this device")


# --------------------------------------------------------------------------------- 1 + 4: grouping is invisible; which kernel ran
@pytest.mark.parametrize("per_flow", [False, True], ids=["one_alignment", "alignment_per_flow"])
@pytest.mark.parametrize("mode", MODES)
def test_batch_equals_every_utterance_decoded_alone(mode, per_flow, monkeypatch):
    need_persist()
    m, cfg = TB.model()
    residual, spk, text, alignment = hard_case(per_flow)
    M = residual.shape[1]
    alone = []
    for b in range(5):
        mel, n = aligned(m, mode, residual, spk, text, alignment, IN_LENS, N_FRAMES, idx=[b], persistent=True)
        assert n.tolist() == [N_FRAMES[b]] and tuple(mel.shape) == (1, M, N_FRAMES[b])
        assert torch.isfinite(mel).all() and float(mel.abs().max()) > 0
        alone.append(mel[0])
    calls = count_calls(monkeypatch)
    nbmax = TB.nbmax()
    for B in (5, 2, 4):
        idx = list(range(B))
        for k in calls:
            calls[k] = 0
        with T64.Watch(True):                                    # stamped frame 0, no failure counted, status word clean
            mel, n = aligned(m, mode, residual, spk, text, alignment, IN_LENS, N_FRAMES, idx=idx, persistent=True)
        assert calls["ft_decode_flow_batch_forced"] == cfg["n_flows"] * math.ceil(B / nbmax), calls
        assert calls["ft_decode_flow"] == calls["ft_decode_flow_batch"] == calls["ft_decode_flow_batch_keys"] == 0, calls
        assert n.dtype == torch.int64 and not n.is_cuda and n.tolist() == N_FRAMES[:B]
        assert tuple(mel.shape) == (B, M, max(N_FRAMES[:B]))
        for b in idx:
            assert torch.equal(mel[b, :, :N_FRAMES[b]], alone[b]), (B, b)
            assert float(mel[b, :, N_FRAMES[b]:].abs().sum()) == 0.0, (B, b)
    if not per_flow:                                             # [B,N,L] is [F,B,N,L] with the same rows for every flow
        mel4, _ = aligned(m, mode, residual, spk, text, torch.stack([alignment] * cfg["n_flows"]), IN_LENS, N_FRAMES, persistent=True)
        assert torch.equal(mel4, mel_of(alone, M))


def mel_of(alone, M):
    out = alone[0].new_zeros(len(alone), M, max(a.shape[1] for a in alone))
    for b, a in enumerate(alone):
        out[b, :, :a.shape[1]] = a
    return out


@pytest.mark.parametrize("mode", MODES)
def test_the_staged_loop_stays_the_default_and_differs_only_in_rounding(mode):
    """persistent=False is the loop of the parent commit (test_gpu_align.py holds it to infer(attns=) bit for bit); the persistent
    path is the same decode in another summation order: close to it, and (documented) not bit-identical"""
    need_persist()
    m, cfg = TB.model()
    residual, spk, text, alignment = hard_case(False)
    with T64.Watch(False):                                       # the default leaves no persistent stage stamps
        ref, n_ref = aligned(m, mode, residual, spk, text, alignment, IN_LENS, N_FRAMES)
    got, n = aligned(m, mode, residual, spk, text, alignment, IN_LENS, N_FRAMES, persistent=True)
    assert n.tolist() == n_ref.tolist() == N_FRAMES and got.shape == ref.shape
    err = float((got - ref).abs().max())
    print("persistent against staged, %s: max difference %.3e, bit-identical: %s" % (mode, err, torch.equal(got, ref)))
    assert err <= 1e-4                                           # what test_infer_vs_reference_golden grants a decode in fp32


@pytest.mark.parametrize("mode", MODES)
def test_alignment_views_at_any_offset_give_the_bits_of_a_fresh_tensor(mode):
    """The launch wants 16-byte aligned rows; the caller's alignment may be a view at any offset: a sliced batch of a larger
    [B', N, L] tensor, one whose N * L is odd so that an utterance starts 4 bytes off, and a slice of a [F', B, N, L] stack whose
    flows then start off a 16-byte boundary.  Default lengths (in_lens = n_frames = None), where no cut makes a copy."""
    need_persist()
    m, cfg = TB.model()
    B, N, Lk = 3, 13, 7                                          # B * N * L = 273: odd
    residual, spk, text = TB.inputs(B, N, Lk, seed=41)
    g = torch.Generator().manual_seed(6)
    big = torch.softmax(torch.randn(cfg["n_flows"] + 1, B + 1, N, Lk, generator=g) * 2, 3).cuda()
    big2 = torch.softmax(torch.randn(cfg["n_flows"] + 1, B, N, Lk, generator=g) * 2, 3).cuda()
    with TB.env(FLOWTRON_MFMA=mode):
        for view in (big[0, 1:], big[1:, 1:], big2[1:]):
            assert not view.is_contiguous() or view.data_ptr() % 16 != 0
            if view.dim() == 4:
                assert any(view[f].data_ptr() % 16 != 0 for f in range(cfg["n_flows"]))
            with T64.Watch(True):
                got, n = m.infer_aligned(residual, spk, text, view, persistent=True)
            ref, n_ref = m.infer_aligned(residual, spk, text, view.clone(), persistent=True)
            assert n.tolist() == n_ref.tolist() == [N] * B and torch.equal(got, ref)
            staged, _ = m.infer_aligned(residual, spk, text, view)
            assert float((got - staged).abs().max()) <= 1e-4     # and the view's own rows were decoded, not a neighbour's


# ------------------------------------------------------------------------------------------------------------- 2: against float64
FCase = namedtuple("FCase", "name in_lens out_lens rows stops poison", defaults=("soft", None, False))
FCASES = (
    [FCase("L%d" % l, [l], [17]) for l in (1, 2, 63, 64, 65, 129, 257, 300, 1000, 1024)]
    + [FCase("N%d" % n, [69], [n]) for n in (1, 7, 8, 9)]
    + [FCase("hard rows", [69], [17], rows="hard"),
       FCase("unnormalised rows", [69], [17], rows="unnormalised"),
       FCase("batch of 5, soft rows", [21] * 5, [17, 12, 17, 9, 14]),
       FCase("ragged batch with poison", [157, 2, 64, 300, 65], [17, 13, 12, 14, 17], poison=True),
       FCase("gate stops at 0, 8, 16", [21, 33, 9], [17, 17, 17], stops=[0, 8, 16]),
       FCase("ragged gate stops with poison", [130, 9, 257, 21, 64], [17, 17, 17, 14, 17], stops=[8, 0, 16, None, 3], poison=True)]
)


def given_rows(kind, n, l, seed):
    """[n, l] fp32 rows: soft = a softmax of random logits; hard = one-hot, monotonic; unnormalised = random non-negative values
    whose sums are not 1.  Row i does not depend on n."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(max(n, 17), l, generator=g)
    if kind == "soft":
        return torch.softmax(r * 2, 1)[:n].contiguous()
    if kind == "unnormalised":
        return (r.abs() * 0.37)[:n].contiguous()
    t = torch.arange(max(n, 17))
    return torch.nn.functional.one_hot(torch.clamp(t * l // 17, max=l - 1), l).float()[:n].contiguous()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fc", FCASES, ids=lambda c: c.name.replace(" ", "_").replace(",", ""))
def test_forced_launch_vs_float64(fc, mode, capsys):
    """AR_Step.infer_batch(forced=): every utterance against its own float64 decode along the same rows, on the V and the
    residual the launch received.  Poison: NaN in the rows' columns and frames behind an utterance's lengths, in its residual
    frames and in its text positions behind them -- none of it may reach an output."""
    need_persist()
    dev = torch.device("cuda", 0)
    gated = fc.stops is not None
    cfg, w, step = T64.flow_setup(False, (), gated)
    _, sd = R.model_sd()
    B, Lmax, Nmax = len(fc.in_lens), max(fc.in_lens), max(fc.out_lens)
    rounding = T64.ROUNDING[mode]
    res, encs, rows = [], [], []
    for b in range(B):
        r, e = R.case_inputs(cfg, sd, 17, fc.in_lens[b], seed=500 + 10 * b)
        res.append(r)
        encs.append(e)
        rows.append(given_rows(fc.rows, 17, fc.in_lens[b], 900 + b))
    fill = float("nan") if fc.poison else 0.0
    x = torch.full((Nmax, B, cfg["n_mel_channels"]), fill)
    text = torch.full((Lmax, B, encs[0].shape[1]), fill)
    forced = torch.full((B, Nmax, Lmax), fill)
    for b in range(B):
        nb, lb = fc.out_lens[b], fc.in_lens[b]
        x[:nb, b] = res[b][:nb]
        text[:lb, b] = encs[b]
        forced[b, :nb, :lb] = rows[b][:nb]
    x, text, forced = x.to(dev), text.to(dev), forced.to(dev)
    KV = [T64.project(step, encs[b].to(dev), mode) for b in range(B)]
    if gated:
        w0 = {k: v for k, v in w.items() if not k.startswith("gate_layer.")}
        free = [R.decode(w0, res[b][:fc.out_lens[b]], KV[b][1], KV[b][1], rounding=rounding, forced=rows[b][:fc.out_lens[b]])["gate_in"]
                for b in range(B)]
        gw, gb = R.design_gate(free, fc.stops)
        w = dict(w, **{"gate_layer.linear_layer.weight": gw, "gate_layer.linear_layer.bias": gb})
        with torch.no_grad():
            step.gate_layer.linear_layer.weight.copy_(gw)
            step.gate_layer.linear_layer.bias.copy_(gb)
        step.gate_threshold = 0.5
    step.attention_layer.temperature = 1.0
    with T64.env(FLOWTRON_MFMA=mode, FLOWTRON_DECODE_PERSIST=1, FLOWTRON_DECODE_BATCH=1):
        with T64.Watch(True):
            out, attn, n = step.infer_batch(x, text, list(fc.out_lens), list(fc.in_lens), forced=forced)
    out, attn = out.cpu(), attn.cpu()
    assert torch.isfinite(out).all() and torch.isfinite(attn).all(), "poison behind an utterance's lengths reached an output"
    assert tuple(attn.shape[1:]) == (B, 1, Lmax)
    nbmax = TB.nbmax()
    for b in range(B):
        nb, lb = fc.out_lens[b], fc.in_lens[b]
        g0 = b - b % nbmax
        kb = step._decode_batch_bufs[(min(nbmax, B - g0), max(fc.out_lens[g0:g0 + nbmax]), Lmax, str(dev))]
        # the group's own buffers hold what its launch received
        assert torch.equal(kb["V"][b - g0, :lb], KV[b][1]) and torch.equal(kb["res"][b - g0, :nb].cpu(), res[b][:nb]), b
        V = KV[b][1]
        kw = dict(gate_threshold=0.5) if gated else {}
        key = ("forced " + fc.name, mode, b)
        ref, d_mel, d_attn = T64.reference(key, w, res[b][:nb], V, V, rounding=rounding, forced=rows[b][:nb], **kw)
        nd = ref["n_done"]
        if gated:
            margin = (ref["gate_logit"] - R.logit_threshold(0.5)).abs().min().item()
            assert margin >= 0.5, margin
            assert nd == (nb if fc.stops[b] is None else fc.stops[b] + 1)
        assert int(n[b]) == nd, (b, n, nd)
        floor = T64.floor_of(key, w, V, V, cfg, res[b], mode, forced=rows[b]) if nd <= 9 else None
        tol_mel, _ = R.tolerance(d_mel, d_attn, floor)
        e_mel = (out[:nd, b].double() - ref["mel"]).abs().max().item()
        with capsys.disabled():
            print("\n[forced f64] %-5s| %-30s [%d: L %4d] frames %3d | mel err %.2e D %.2e ratio %6.2f"
                  % (mode, fc.name, b, lb, nd, e_mel, tol_mel / R.MARGIN, e_mel / (tol_mel / R.MARGIN)), flush=True)
        assert e_mel <= tol_mel, "mel: max error %.3e > 10 x D = %.3e" % (e_mel, tol_mel)
        assert torch.equal(attn[:nd, b, 0, :lb], rows[b][:nd]), "the written attention rows are not the given rows"
        assert not out[nd:, b].any() and not attn[nd:, b].any(), "rows behind utterance %d's end" % b
        assert not attn[:, b, 0, lb:].any(), "attention columns behind utterance %d's keys" % b


# ---------------------------------------------------------------------------------- 3: own attention reproduces the decode
@pytest.mark.parametrize("mode", MODES)
def test_own_attention_reproduces_the_free_running_decode(mode, capsys):
    """A batch decoded free-running on the batched persistent path, then again along the attention rows it returned.  Flow by
    flow on shared inputs: the forced decode of a flow gets the frames the free-running decode of that flow got (the last flow's
    are the caller's residual in both; the first flow's are the free run's where the last flow did not come out bit-identical)
    and must agree with it within decode_ref64.tolerance of that flow's float64 decode along those rows.  That bound is defined
    per flow on shared inputs, so it does not carry over to the end-to-end mel, where the second flow decoded starts from frames
    that may differ in the last bits; end to end the two mels are held to 1e-4, what test_infer_vs_reference_golden grants a whole
    decode against the reference implementation (both are whole decodes of the same residual along the same attention).
    Outcome on the MI355X (reported, not asserted: the compiler may schedule the two instantiations' FMAs differently):
    fp32 weights: bit-identical, every flow and utterance; bf16 weight images: NOT bit-identical, flow-level differences of
    1.2e-7 .. 1.8e-7 = up to 1.6 D (profiles/decode_aligned_newtests.log)."""
    need_persist()
    m, cfg = TB.model()
    B, N, Lk = 3, 20, 23
    residual, spk, text = TB.inputs(B, N, Lk, seed=33)
    steps = [f.ar_step if hasattr(f, "ar_step") else f for f in m.flows]
    rec = {}

    def recorder(tag, f, st, orig):
        def infer_batch(x, enc, lens, in_lens=None, forced=None):
            o = orig(x, enc, lens, in_lens, forced)
            kb = st._decode_batch_bufs[(B, N, Lk, str(x.device))]
            rec[(tag, f)] = dict(x=x.clone(), enc=enc.clone(), V=kb["V"].clone(), out=o[0].clone(), attn=o[1].clone(), forced=forced)
            return o
        return infer_batch

    def run(tag, fn):
        try:
            for f, st in enumerate(steps):
                st.infer_batch = recorder(tag, f, st, type(st).infer_batch.__get__(st))
            with TB.env(FLOWTRON_MFMA=mode, FLOWTRON_DECODE_BATCH=1, FLOWTRON_DECODE_PERSIST=1):
                return fn()
        finally:
            for st in steps:
                del st.infer_batch

    F_ = cfg["n_flows"]
    with T64.Watch(True):
        mel, aws, lens = run("free", lambda: m.infer(residual, spk, text, gate_threshold=1.0, return_lengths=True))
    assert lens.tolist() == [N] * B and len(aws) == F_
    # aws[i] belongs to flow F - 1 - i (the decode order) and is in that flow's own time order: natural time for infer_aligned
    alignment = torch.stack([torch.cat(aws[F_ - 1 - f], 1) for f in range(F_)])          # [F, B, N, L]
    alignment = torch.stack([torch.flip(a, (1,)) if f % 2 == 1 else a for f, a in enumerate(alignment)])
    with T64.Watch(True):
        mel2, n2 = run("forced", lambda: m.infer_aligned(residual, spk, text, alignment, persistent=True))
    assert n2.tolist() == [N] * B and mel2.shape == mel.shape
    same = torch.equal(mel2, mel)
    e2e = float((mel2 - mel).abs().max())
    with capsys.disabled():
        print("\n[own attention] %s: end-to-end mel difference %.3e (bound 1e-4)" % (mode, e2e), flush=True)
    assert e2e <= 1e-4, e2e
    rounding = T64.ROUNDING[mode]
    from oracle import flowtron_oracle as O
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    worst = 0.0
    for f in reversed(range(F_)):
        fr, fo = rec[("free", f)], rec[("forced", f)]
        assert torch.equal(fo["forced"][:, :N], fr["attn"][:, :, 0].transpose(0, 1)), f     # the rows handed over are the free run's
        out = fo["out"]
        if not torch.equal(fo["x"], fr["x"]):                    # an earlier flow differed in the last bits: decode on the free run's frames
            with TB.env(FLOWTRON_MFMA=mode, FLOWTRON_DECODE_BATCH=1, FLOWTRON_DECODE_PERSIST=1):
                out = steps[f].infer_batch(fr["x"], fr["enc"], [N] * B, [Lk] * B, forced=fo["forced"])[0]
        w = R.flow_weights(sd, O.flow_prefix(f))
        for b in range(B):
            rows = fr["attn"][:, b, 0].cpu()
            ref, d_mel, d_attn = T64.reference(("own attention", mode, f, b), w, fr["x"][:, b].cpu(), fr["V"][b].cpu(), fr["V"][b].cpu(),
                                               rounding=rounding, forced=rows, gate_threshold=2.0)
            tol_mel, _ = R.tolerance(d_mel, d_attn)
            e = (out[:, b].double().cpu() - fr["out"][:, b].double().cpu()).abs().max().item()
            e_ref = (out[:, b].double().cpu() - ref["mel"]).abs().max().item()
            worst = max(worst, e / (tol_mel / R.MARGIN))
            with capsys.disabled():
                print("\n[own attention] %-5s flow %d utterance %d | forced - free %.2e, forced - float64 %.2e, D %.2e"
                      % (mode, f, b, e, e_ref, tol_mel / R.MARGIN), flush=True)
            assert e <= tol_mel and e_ref <= tol_mel, (f, b, e, e_ref, tol_mel)
    with capsys.disabled():
        print("\n[own attention] %s: the decode along its own attention is %sbit-identical to the free-running decode "
              "(largest flow-level difference %.2f D)" % (mode, "" if same else "NOT ", worst), flush=True)


# ------------------------------------------------------------------------------------------------------------------ 5: round trip
def test_round_trip_with_persistent_decode(capsys):
    """test_gpu_align.py's round trip at full width (the persistent geometry): mel -> alignments -> infer_aligned(z, the per-flow
    soft attention, persistent=True) gives mel back.  Bound, as there: what the CPU oracle's own forward followed by its forced
    infer deviates on the same case, plus 1e-4."""
    from oracle import flowtron_oracle as O
    from oracle import synth
    need_persist()
    m, cfg = TB.model(seed=5, gate_spread=False, n_speakers=3)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    sb = synth.make_batch(cfg, [30, 17, 21], [9, 7, 5], seed=31, with_prior=False)            # sorted by text length
    order = [2, 0, 1]
    idx = torch.tensor(order)
    b = {k: sb[k][idx].cuda() for k in ("mel", "speaker_ids", "text", "in_lens", "out_lens")}
    il, ol = b["in_lens"].tolist(), b["out_lens"].tolist()
    with TB.env(FLOWTRON_MFMA="f32"):
        z, attn, _ = m.alignments(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
        assert float((z - b["mel"]).abs().max()) > 1e-2                    # the flows are not the identity
        with T64.Watch(True):
            mel, lengths = m.infer_aligned(z, b["speaker_ids"], b["text"], attn, in_lens=il, n_frames=ol, persistent=True)
    assert lengths.tolist() == ol
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
    with capsys.disabled():
        print("\n[round trip, persistent] oracle deviation %.3e, device deviation %.3e" % (dev_o, dev_d), flush=True)
    assert dev_d <= dev_o + 1e-4, (dev_d, dev_o)


# ------------------------------------------------------------------------------------------------------- 6: routing and refusals
@pytest.mark.parametrize("case", ["cumm", "depth3", "persist_off", "batch_off"])
def test_outside_the_geometry_or_switched_off_it_is_the_staged_loop(case, monkeypatch):
    over = {"cumm": dict(use_cumm_attention=True), "depth3": dict(n_lstm_layers=3)}.get(case, {})
    sw = {"persist_off": dict(FLOWTRON_DECODE_PERSIST=0), "batch_off": dict(FLOWTRON_DECODE_BATCH=0)}.get(case, {})
    m, cfg = TB.model(seed=9, gate_spread=False, **over)
    B, N, Lk = 3, 12, 15
    residual, spk, text = TB.inputs(B, N, Lk, seed=11)
    g = torch.Generator().manual_seed(2)
    alignment = torch.softmax(torch.randn(B, N, Lk, generator=g) * 2, 2).cuda()
    il, nf = [15, 9, 12], [12, 7, 10]
    with TB.env(**sw):
        ref, n_ref = aligned(m, "f32", residual, spk, text, alignment, il, nf)
        calls = count_calls(monkeypatch)
        got, n = aligned(m, "f32", residual, spk, text, alignment, il, nf, persistent=True)
    assert calls["ft_decode_flow_batch_forced"] == 0 and calls["ft_decode_flow"] == B * cfg["n_flows"], calls
    assert torch.equal(got, ref) and n.tolist() == n_ref.tolist() == nf


def test_entry_refuses_without_launching():
    """nb = 0, nb = max + 1 and no rows: FT_EUNSUPPORTED before any pointer is looked at (none is valid here)"""
    import ctypes as C
    from flowtron_amd import _lib as L
    lib = L.lib()
    a = L.DecodeArgs()
    a.N, a.L, a.H, a.A, a.M, a.E, a.n_layers, a.temperature = 10, 23, 1024, 640, 80, 1, 2, 1.0
    a.forced = 1 << 20
    for nb in (0, lib.ft_decode_batch_max() + 1):
        assert lib.ft_decode_flow_batch_forced(C.byref(L.DecodeBatchArgs(a, nb, None, 0)), None, None) == -3
    a.forced = None
    assert lib.ft_decode_flow_batch_forced(C.byref(L.DecodeBatchArgs(a, 2, None, 0)), None, None) == -3
    assert b"ft_decode_flow_batch_forced" in lib.ft_last_error()
