"""Batched persistent decode (csrc/decode_batch.hip dec_persist_batch_k through Flowtron.infer): a batch decodes flow by flow in
groups of up to ft_decode_batch_max() utterances per launch, and every utterance must come out bit for bit as the
utterance-by-utterance loop (FLOWTRON_DECODE_BATCH=0) decodes it -- mel and every attention row on its frames, zeros behind its
stop.  Full-width synthetic 2-flow models with fp32 weights (the default, outside autocast) and bf16 weight images."""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_MODELS = {}


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def model(seed=17, gate_spread=True, **over):
    """full-width model; with gate_spread the gate logits spread about one unit around -2, so utterances stop at different frames"""
    import flowtron
    from oracle import synth
    key = (seed, gate_spread, tuple(sorted(over.items())))
    if key not in _MODELS:
        cfg = dict(synth.DEFAULT_MODEL_CONFIG, n_text=60, n_flows=2, **over)
        sd = synth.make_state_dict(cfg, seed=seed)
        if gate_spread:
            gk = [k for k in sd if "gate_layer" in k and k.endswith("weight")][0]
            g = torch.Generator().manual_seed(4)
            sd[gk] = torch.randn(sd[gk].shape, generator=g) * 0.05
            sd[gk.replace("weight", "bias")] = torch.full_like(sd[gk.replace("weight", "bias")], -2.0)
        m = flowtron.Flowtron(**cfg)
        m.load_state_dict(sd)
        _MODELS[key] = (m.cuda().eval(), cfg)
    return _MODELS[key]


def inputs(B, N, Lk, seed=0, n_speakers=1):
    g = torch.Generator().manual_seed(seed)
    residual = (torch.randn(B, 80, N, generator=g) * 0.5).cuda()
    text = torch.randint(1, 60, (B, Lk), generator=g).cuda()
    spk = (torch.arange(B) % n_speakers).cuda()
    return residual, spk, text


def infer(m, residual, spk, text, batch, mode, **kw):
    with env(FLOWTRON_DECODE_BATCH=int(batch), FLOWTRON_MFMA=mode):
        return m.infer(residual, spk, text, **kw)


def lengths(mel, B):
    """frames of each utterance: its last frame with any non-zero value + 1 (decoded frames are never exactly zero)"""
    nz = mel.abs().amax(1) != 0                                  # [B, n]
    return [int(nz[b].nonzero().max()) + 1 if bool(nz[b].any()) else 0 for b in range(B)]


def assert_same(got, ref, B, n_flows, lens=None):
    mel, attns = got
    rmel, rattns = ref
    assert mel.shape == rmel.shape, (mel.shape, rmel.shape)
    assert torch.equal(mel, rmel)                                # values on each utterance's frames, exact zeros behind its stop
    lens = lens or lengths(rmel, B)
    assert mel.shape[2] == max(lens)
    for f in range(n_flows):
        assert len(attns[f]) == len(rattns[f]) == max(lens)
        a, r = torch.stack(attns[f]), torch.stack(rattns[f])     # [n, B, 1, L]
        assert torch.equal(a, r), f
        for b in range(B):
            assert float(a[lens[b]:, b].abs().max()) == 0.0 if lens[b] < max(lens) else True


def nbmax():
    from flowtron_amd import _lib as L
    return L.lib().ft_decode_batch_max()


_THR = {}


def separating_threshold(mode, B, N, Lk):
    """a gate threshold at which the utterances stop at different frames (the search of
    test_gated_batch_decode_equals_the_utterances_decoded_alone, on the utterance loop)"""
    if mode not in _THR:
        m, _ = model()
        residual, spk, text = inputs(B, N, Lk, seed=3)
        for thr in (0.03, 0.05, 0.08, 0.12, 0.16, 0.2, 0.25, 0.3, 0.4, 0.5):
            lens = lengths(infer(m, residual, spk, text, False, mode, gate_threshold=thr)[0], B)
            if len(set(lens)) > 2 and min(lens) < N:
                break
        else:
            pytest.fail("no threshold separated the stops: %r" % (lens,))
        _THR[mode] = thr
    return _THR[mode]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("gated", [True, False])
def test_batch_decode_is_bit_identical_to_the_utterance_loop(mode, gated):
    m, cfg = model()
    N, Lk = 40, 23
    Bs = (2, 4, nbmax() + 1)
    thr = separating_threshold(mode, max(Bs), N, Lk) if gated else 1.0
    residual, spk, text = inputs(max(Bs), N, Lk, seed=3)
    for B in Bs:
        r, s, t = residual[:B], spk[:B], text[:B]
        ref = infer(m, r, s, t, False, mode, gate_threshold=thr)
        got = infer(m, r, s, t, True, mode, gate_threshold=thr)
        assert_same(got, ref, B, cfg["n_flows"])
        if gated and B == max(Bs):
            assert len(set(lengths(ref[0], B))) > 1


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("Lk", [1, 23, 129, 257, 300, 1000])
def test_batch_decode_text_lengths_and_speakers(mode, Lk):
    """across the resident key / value limits of the single-utterance kernel (bf16 256, fp32 128 symbols) and past 512 symbols (the
    second granule pair of every thread in the score / context gathers); a speaker per utterance"""
    m, cfg = model(seed=5, gate_spread=False, n_speakers=3)
    residual, spk, text = inputs(3, 24, Lk, seed=Lk, n_speakers=3)
    ref = infer(m, residual, spk, text, False, mode, gate_threshold=1.0)
    got = infer(m, residual, spk, text, True, mode, gate_threshold=1.0)
    assert_same(got, ref, 3, cfg["n_flows"], lens=[24] * 3)


def count_calls(monkeypatch):
    from flowtron_amd import _lib as L
    lib = L.lib()
    calls = {"single": 0, "batch": 0}
    for name, k in (("ft_decode_flow", "single"), ("ft_decode_flow_batch", "batch")):
        fn = getattr(lib, name)

        def shim(*a, _fn=fn, _k=k):
            calls[_k] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, shim)
    return calls


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_one_batched_launch_per_flow(mode, monkeypatch):
    from flowtron_amd import ops
    m, cfg = model()
    residual, spk, text = inputs(nbmax() + 1, 20, 23, seed=7)
    calls = count_calls(monkeypatch)
    infer(m, residual[:4], spk[:4], text[:4], True, mode, gate_threshold=1.0)
    assert calls == {"single": 0, "batch": cfg["n_flows"]}, calls
    assert ops.check_persist_status(raise_on_failure=False)
    calls.update(single=0, batch=0)
    infer(m, residual, spk, text, True, mode, gate_threshold=1.0)   # NBMAX + 1: a group of NBMAX and a group of one per flow
    assert calls == {"single": cfg["n_flows"], "batch": cfg["n_flows"]}, calls
    assert ops.check_persist_status(raise_on_failure=False)


@pytest.mark.parametrize("case", ["prior", "cumm", "depth3"])
def test_other_decodes_keep_the_utterance_loop(case, monkeypatch):
    """attention prior, cumulative attention, three decoder layers: no batched launch, results unchanged"""
    over = {"cumm": dict(use_cumm_attention=True), "depth3": dict(n_lstm_layers=3)}.get(case, {})
    mode = "f32"
    m, cfg = model(seed=9, gate_spread=False, **over)
    B, N, Lk = 3, 12, 15
    residual, spk, text = inputs(B, N, Lk, seed=11)
    kw = dict(gate_threshold=1.0)
    if case == "prior":
        g = torch.Generator().manual_seed(2)
        kw["attn_prior"] = torch.rand(B, N, Lk, generator=g).cuda() + 0.1
    ref = infer(m, residual, spk, text, False, mode, **kw)
    calls = count_calls(monkeypatch)
    got = infer(m, residual, spk, text, True, mode, **kw)
    assert calls["batch"] == 0 and calls["single"] == B * cfg["n_flows"], calls
    assert_same(got, ref, B, cfg["n_flows"], lens=[N] * B)
