"""Sentences of different lengths in one batched Flowtron.infer call (in_lens / out_lens / return_lengths): utterance b must come out
bit for bit as infer(residual[b:b+1, :, :out_lens[b]], speaker_ids[b:b+1], text[b:b+1, :in_lens[b]]) decodes it alone -- its mel
frames, its attention columns < in_lens[b] on its frames, exact zeros everywhere else, and its frame count -- on the batched
persistent launch (csrc/decode_batch.hip dec_persist_batch_k with a key count per utterance, ft_decode_flow_batch_keys) and on every
configuration that keeps the utterance loop.  Full-width synthetic 2-flow models with fp32 weights and bf16 weight images."""
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


def model(seed=17, gate_spread=True, small=False, **over):
    """with gate_spread the gate logits spread about one unit around -2, so utterances stop at different frames"""
    import flowtron
    from oracle import synth
    key = (seed, gate_spread, small, tuple(sorted(over.items())))
    if key not in _MODELS:
        base = synth.SMALL_MODEL_CONFIG if small else dict(synth.DEFAULT_MODEL_CONFIG, n_text=60)
        cfg = dict(base, n_flows=2, **over)
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


def inputs(B, N, Lk, seed=0, n_text=60, n_speakers=1):
    g = torch.Generator().manual_seed(seed)
    residual = (torch.randn(B, 80, N, generator=g) * 0.5).cuda()
    text = torch.randint(1, n_text, (B, Lk), generator=g).cuda()
    spk = (torch.arange(B) % n_speakers).cuda()
    return residual, spk, text


def infer(m, *a, batch=True, mode="f32", **kw):
    with env(FLOWTRON_DECODE_BATCH=int(batch), FLOWTRON_MFMA=mode):
        return m.infer(*a, **kw)


def alone(m, residual, spk, text, il, ol, mode="f32", prior=None, **kw):
    """each utterance decoded on its own, trimmed to its lengths"""
    return [infer(m, residual[b:b + 1, :, :ol[b]], spk[b:b + 1], text[b:b + 1, :il[b]], mode=mode,
                  attn_prior=None if prior is None else prior[b:b + 1, :ol[b], :il[b]], **kw) for b in range(len(il))]


def assert_ragged(got, refs, il, n_flows):
    mel, attns, lens = got
    B, Lt = mel.shape[0], attns[0][0].shape[2]
    n = [int(r[0].shape[2]) for r in refs]
    assert lens.dtype == torch.int64 and lens.device.type == "cpu" and lens.tolist() == n, (lens, n)
    assert tuple(mel.shape) == (B, 80, max(n)), mel.shape
    for f in range(n_flows):
        assert len(attns[f]) == max(n)
        a = torch.stack(attns[f])                                # [max n, B, 1, Lt]
        assert tuple(a.shape) == (max(n), B, 1, Lt)
        for b in range(B):
            r = torch.stack(refs[b][1][f])                       # [n_b, 1, 1, il_b]
            assert tuple(r.shape) == (n[b], 1, 1, il[b]), (f, b, r.shape)
            assert torch.equal(a[:n[b], b, 0, :il[b]], r[:, 0, 0]), (f, b)
            assert not a[:n[b], b, 0, il[b]:].any(), (f, b)      # columns behind its text
            assert not a[n[b]:, b].any(), (f, b)                 # rows behind its end
    for b in range(B):
        assert torch.equal(mel[b, :, :n[b]], refs[b][0][0]), b
        assert not mel[b, :, n[b]:].any(), b


_THR = {}


def separating_threshold(m, residual, spk, text, il, ol, mode):
    """a gate threshold at which the alone decodes stop at different frames, some before their out_lens"""
    if mode not in _THR:
        for thr in (0.03, 0.05, 0.08, 0.12, 0.16, 0.2, 0.25, 0.3, 0.4, 0.5):
            n = [int(r[0].shape[2]) for r in alone(m, residual, spk, text, il, ol, mode, gate_threshold=thr)]
            if len(set(n)) > 2 and any(n[b] < ol[b] for b in range(len(n))):
                break
        else:
            pytest.fail("no threshold separated the stops: %r" % (n,))
        _THR[mode] = thr
    return _THR[mode]


# text lengths: one symbol, mid-way through the second 128-position stride of the score stage, past the resident key rows of both
# precisions, past 512 (the second granule pair of the score gather), and near 1000
IL6 = [200, 1, 997, 57, 513, 130]
OL6 = [31, 12, 24, 36, 7, 19]
N6, L6 = 36, 1000


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("gated", [True, False])
def test_ragged_batch_equals_each_utterance_decoded_alone(mode, gated):
    m, cfg = model()
    residual, spk, text = inputs(6, N6, L6, seed=3)
    thr = separating_threshold(m, residual, spk, text, IL6, OL6, mode) if gated else 1.0
    refs = alone(m, residual, spk, text, IL6, OL6, mode, gate_threshold=thr)
    if gated:
        assert any(int(refs[b][0].shape[2]) < OL6[b] for b in range(6))
    # B 6: a group of 4 and a group of 2, both batched launches (device lengths); B 5: a group of 4 and a single (host tensors)
    got = infer(m, residual, spk, text, mode=mode, gate_threshold=thr, in_lens=torch.tensor(IL6).cuda(), out_lens=OL6,
                return_lengths=True)
    assert_ragged(got, refs, IL6, cfg["n_flows"])
    got = infer(m, residual[:5], spk[:5], text[:5], mode=mode, gate_threshold=thr, in_lens=torch.tensor(IL6[:5]),
                out_lens=torch.tensor(OL6[:5], dtype=torch.int32), return_lengths=True)
    assert_ragged(got, refs[:5], IL6[:5], cfg["n_flows"])


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_padding_is_inert(mode):
    """token ids behind in_lens and residual frames behind out_lens are never read"""
    m, cfg = model()
    il, ol = [40, 3, 129, 77, 90], [20, 9, 14, 25, 11]
    residual, spk, text = inputs(5, 25, 140, seed=8)
    g = torch.Generator().manual_seed(1)
    text_z, text_r = text.clone(), text.clone()
    res_z, res_r = residual.clone(), residual.clone()
    for b in range(5):
        text_z[b, il[b]:] = 0
        text_r[b, il[b]:] = torch.randint(1, 60, (140 - il[b],), generator=g).cuda()
        res_z[b, :, ol[b]:] = 0
        res_r[b, :, ol[b]:] = (torch.randn(80, 25 - ol[b], generator=g) * 3.0).cuda()
    kw = dict(mode=mode, gate_threshold=0.12, in_lens=il, out_lens=ol, return_lengths=True)
    for batch in (True, False):
        a = infer(m, res_z, spk, text_z, batch=batch, **kw)
        b_ = infer(m, res_r, spk, text_r, batch=batch, **kw)
        assert torch.equal(a[0], b_[0]) and torch.equal(a[2], b_[2]), batch
        for f in range(cfg["n_flows"]):
            assert torch.equal(torch.stack(a[1][f]), torch.stack(b_[1][f])), (batch, f)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_full_lengths_change_nothing(mode):
    m, cfg = model()
    B, N, Lk = 5, 22, 150
    residual, spk, text = inputs(B, N, Lk, seed=5)
    for batch in (True, False):
        ref = infer(m, residual, spk, text, batch=batch, mode=mode, gate_threshold=0.12)
        got = infer(m, residual, spk, text, batch=batch, mode=mode, gate_threshold=0.12, in_lens=[Lk] * B,
                    out_lens=torch.full((B,), N).cuda(), return_lengths=True)
        assert torch.equal(got[0], ref[0]), batch
        for f in range(cfg["n_flows"]):
            assert len(got[1][f]) == len(ref[1][f])
            assert torch.equal(torch.stack(got[1][f]), torch.stack(ref[1][f])), (batch, f)
        nz = ref[0].abs().amax(1) != 0                           # decoded frames are never exactly zero
        assert got[2].tolist() == [int(nz[b].nonzero().max()) + 1 for b in range(B)]
    # B = 1 through the same slicing
    ref = infer(m, residual[:1], spk[:1], text[:1], mode=mode, gate_threshold=1.0)
    got = infer(m, residual[:1], spk[:1], text[:1], mode=mode, gate_threshold=1.0, in_lens=[Lk], out_lens=[N], return_lengths=True)
    assert torch.equal(got[0], ref[0]) and got[2].tolist() == [N]
    got = infer(m, residual[:1], spk[:1], text[:1], mode=mode, gate_threshold=1.0, in_lens=[31], out_lens=[9], return_lengths=True)
    assert_ragged(got, alone(m, residual[:1], spk[:1], text[:1], [31], [9], mode, gate_threshold=1.0), [31], cfg["n_flows"])


@pytest.mark.parametrize("case", ["prior", "depth3", "cumm"])
def test_loop_configurations_get_the_lengths_too(case, monkeypatch):
    """small model (the utterance loop by geometry), an inference-time prior, three decoder layers, cumulative attention"""
    over = {"depth3": dict(n_lstm_layers=3), "cumm": dict(use_cumm_attention=True)}.get(case, {})
    m, cfg = model(seed=9, small=True, **over)
    B, N, Lk = 4, 16, 21
    il, ol = [21, 5, 13, 1], [16, 3, 11, 8]
    residual, spk, text = inputs(B, N, Lk, seed=11, n_text=40, n_speakers=3)
    prior = None
    if case == "prior":
        g = torch.Generator().manual_seed(2)
        prior = torch.rand(B, N, Lk, generator=g).cuda() + 0.1
    refs = alone(m, residual, spk, text, il, ol, prior=prior, gate_threshold=0.3)
    calls = count_calls(monkeypatch)
    got = infer(m, residual, spk, text, gate_threshold=0.3, in_lens=il, out_lens=ol, attn_prior=prior, return_lengths=True)
    assert calls["batch"] == calls["keys"] == 0 and calls["single"] == B * cfg["n_flows"], calls
    assert_ragged(got, refs, il, cfg["n_flows"])


def count_calls(monkeypatch):
    from flowtron_amd import _lib as L
    lib = L.lib()
    calls = {"single": 0, "batch": 0, "keys": 0}
    for name, k in (("ft_decode_flow", "single"), ("ft_decode_flow_batch", "batch"), ("ft_decode_flow_batch_keys", "keys")):
        fn = getattr(lib, name)

        def shim(*a, _fn=fn, _k=k):
            calls[_k] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, shim)
    return calls


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_one_ragged_launch_per_flow_and_group(mode, monkeypatch):
    from flowtron_amd import ops
    m, cfg = model()
    nf = cfg["n_flows"]
    residual, spk, text = inputs(6, 20, 300, seed=7)
    il, ol = [300, 12, 150, 7, 260, 33], [20, 15, 9, 18, 20, 4]
    calls = count_calls(monkeypatch)
    infer(m, residual, spk, text, mode=mode, gate_threshold=1.0, in_lens=il, out_lens=ol)
    assert calls == {"single": 0, "batch": 0, "keys": 2 * nf}, calls           # groups of 4 and 2
    assert ops.check_persist_status(raise_on_failure=False)
    calls.update(single=0, batch=0, keys=0)
    infer(m, residual[:5], spk[:5], text[:5], mode=mode, gate_threshold=1.0, in_lens=il[:5], out_lens=ol[:5])
    assert calls == {"single": nf, "batch": 0, "keys": nf}, calls             # a group of 4 and a single
    # a padded text longer than the batch kernel's 1024 positions whose sentences all fit: the batched launch, trimmed
    calls.update(single=0, batch=0, keys=0)
    residual, spk, text = inputs(3, 10, 1100, seed=9)
    il, ol = [1000, 50, 700], [10, 6, 8]
    got = infer(m, residual, spk, text, mode=mode, gate_threshold=1.0, in_lens=il, out_lens=ol, return_lengths=True)
    assert calls == {"single": 0, "batch": 0, "keys": nf}, calls
    assert_ragged(got, alone(m, residual, spk, text, il, ol, mode, gate_threshold=1.0), il, nf)
    assert ops.check_persist_status(raise_on_failure=False)


def test_bad_lengths_raise_before_any_launch(monkeypatch):
    m, _ = model()
    residual, spk, text = inputs(3, 10, 20, seed=1)
    calls = count_calls(monkeypatch)
    bad = [dict(in_lens=[5, 5]), dict(out_lens=[5, 5, 5, 5]), dict(in_lens=[5, 0, 5]), dict(in_lens=[5, 21, 5]),
           dict(out_lens=[10, 11, 1]), dict(out_lens=[0, 1, 1]), dict(in_lens=torch.tensor([5.0, 5.0, 5.0]).cuda()),
           dict(out_lens=torch.tensor([[5, 5, 5]])), dict(in_lens=[5, 5, 5], out_lens=[10, 10, 10], attns=[[], []])]
    for kw in bad:
        with pytest.raises(ValueError):
            infer(m, residual, spk, text, **kw)
    with pytest.raises(ValueError, match="one utterance at a time"):
        infer(m, residual, spk, text, attns=[[], []])
    assert calls == {"single": 0, "batch": 0, "keys": 0}, calls
