"""Every decode kernel against tests/decode_ref64.py: the float64 restatement of one flow's decode with that decoder's own
operand rounding (none in fp32 weight mode; the ten bf16 weight images in the 16-bit modes, FT_F16 included).

Decoders: the staged chain with fp32 weights (hipGraph on and off) and with bf16 images, the one-launch persistent decode in
both precisions (csrc/decode.hip), the batched persistent launch with one text length (ft_decode_flow_batch) and with a key
count per utterance (ft_decode_flow_batch_keys, csrc/decode_batch.hip), all selected the way a caller selects them
(FLOWTRON_MFMA, FLOWTRON_DECODE_PERSIST, use_graph, AR_Step.infer / infer_batch, Flowtron.infer).  A case outside a persistent
kernel's geometry is routed by the library to the staged chain; its row says so.

Each flow is checked on ITS OWN inputs: the reference takes the K and V the kernel received (AR_Step's buffers) and, in the
2-flow test, the residual the previous flow's kernel produced and the encoder output the GPU computed.  Neither the projections'
operand rounding nor an earlier flow's error enters.

Tolerance (decode_ref64.tolerance): per case D_mel, D_attn = the largest deviation of oracle.ar_step_infer IN FP32 ON THE CPU
from the float64 reference, on the same rounded weights and the same K, V -- the reference implementation's own arithmetic noise
(about 2e-7 / 1e-8 at the bench shape).  A kernel is held to 10 x D on every element of mel and of attention separately: the
kernels sum in another order and use the v_exp_f32 / v_rcp_f32 activation forms.  A case that produces at most 9 frames takes
the larger of its D and the D of the ungated 17-frame decode of the same configuration (a handful of frames deviates by a few
ulps of luck; a gate stop at frame 0 is a 1-frame case).  Nothing is stored; every row prints max error / D.

Attention rows: >= 0, and their sum within rowsum_bound(L) = (ceil(L / 256) + 10) x 2^-24 of the reference's row sum (1 to
float64 rounding, or a forced row's own sum): the summation and division roundings of the kernels' fp32 normalisation, derived
at rowsum_bound -- the element tolerance is below the rounding of a sum near 1 and cannot serve.  Every row prints its row-sum
error.  What infer_batch returns is exactly zero behind an utterance's keys and frames.

Which kernel ran is proved per row (class Watch): a row that asks for a persistent kernel inside its geometry must leave that
kernel's stage stamps and no counted failure (the library re-decodes a failed launch on the staged chain by itself, which would
otherwise pass unseen); every other row must leave none.  Whether the persistent kernels exist on the device is decided once,
before the first decode.  The summary lists the rows the library routed to the staged chain apart from those a persistent
kernel took.

Measured on the MI355X, worst max error / D over all cases, mel | attention (bound 10; 151 rows, 108 s for the file):
    f32 staged, hipGraph on and off  1.35 | 1.54      f32 persistent   1.35 | 1.54      f32 batched persistent   1.35 | 0.89
    bf16 staged                      1.41 | 1.13      bf16 persistent  1.48 | 1.13      bf16 batched persistent  1.54 | 0.93
    FT_F16 mode staged               1.10 | 0.36      FT_F16 mode persistent 1.10 | 0.63
With ROUNDING["bf16"] = None the bf16 rows fail at the bench shape: mel 2.02e-4 = 1120 x D (the float64 prediction: 2.02e-4)."""
import contextlib
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import decode_ref64 as R

pytestmark = pytest.mark.gpu

SENT = -77.25            # pre-filled where the ABI says "not written"
Decoder = namedtuple("Decoder", "name mode persist graph")
DECODERS = [
    Decoder("f32 staged, hipGraph", "f32", 0, True),
    Decoder("f32 staged, no graph", "f32", 0, False),
    Decoder("f32 persistent", "f32", 1, True),
    Decoder("bf16 staged", "bf16", 0, True),
    Decoder("bf16 persistent", "bf16", 1, True),
]
F16_DECODERS = [Decoder("f16 mode staged", "f16", 0, True), Decoder("f16 mode persistent", "f16", 1, True)]
ROUNDING = {"f32": None, "bf16": torch.bfloat16, "f16": torch.bfloat16}      # FT_F16 decodes from the bf16 images too

_CASE_FIELDS = "name N Lk small over temperature stop prior forced"
Case = namedtuple("Case", _CASE_FIELDS, defaults=(17, 69, False, (), 1.0, "nogate", False, False))
CASES = (
    [Case("bench shape L69 N400", N=400)]
    + [Case("L%d" % l, Lk=l) for l in (1, 2, 63, 64, 65, 157, 1000, 1024, 1025)]
    + [Case("N%d" % n, N=n) for n in (1, 7, 8, 9, 17)]
    + [Case("temperature 0.7", temperature=0.7)]
    + [Case("gate stop %s" % ("never" if s is None else "at frame %d" % s), stop=s) for s in (0, 8, 16, None)]
    + [Case("prior rows", prior=True), Case("forced alignment", forced=True),
       Case("cumulative attention H1024", over=(("use_cumm_attention", True),)),
       Case("cumulative attention H64", small=True, Lk=23, over=(("use_cumm_attention", True),)),
       Case("depth 1", over=(("n_lstm_layers", 1),)), Case("depth 3", over=(("n_lstm_layers", 3),))]
)
WORST = {}


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


def dec_env(dec):
    return env(FLOWTRON_MFMA=dec.mode, FLOWTRON_DECODE_PERSIST=dec.persist, FLOWTRON_DECODE_BATCH=1, FLOWTRON_DECODE_GRAPH=int(dec.graph))


def persistent_geometry(cfg, Lk, case=None):
    """the geometry dec_persist_k / dec_persist_batch_k accept (ft_decode_flow, decode.hip:949)"""
    plain = case is None or not (case.prior or case.forced)
    return (cfg["n_hidden"] == 1024 and cfg["n_attn_channels"] == 640 and cfg["n_mel_channels"] == 80 and cfg["n_lstm_layers"] == 2
            and not cfg["use_cumm_attention"] and Lk <= 1024 and plain)


_AVAILABLE = []


def persistent_available():
    """Decided ONCE, by the device's self-test before this file's first decode -- never by a launch of this file that failed."""
    from flowtron_amd import ops
    if not _AVAILABLE:
        _AVAILABLE.append(bool(ops.persist_usable(torch.device("cuda", 0))))
    return _AVAILABLE[0]


def need_persist(dec):
    if dec.persist and not persistent_available():
        pytest.skip("persistent kernels not usable on this device")


def _failures():
    from flowtron_amd import ops
    return sum(st.failures for st in ops._PERSIST.values())


class Watch:
    """Around the infer / infer_batch call of a row: proves which kernel decoded it.
    The library hides a persistent launch that does not complete: AR_Step.infer / infer_batch read the status word themselves, clear
    it, switch the device to the staged kernels and decode again (flowtron_amd.decode.launch_or_staged), so a status check afterwards sees
    nothing.  What cannot be hidden: ops' failure counter, persist_usable() turning False, and the stage stamps that only
    dec_persist_k / dec_persist_batch_k write into the ft_decode_debug_prof buffer (decode.hip:561-562, decode_batch.hip:233-234;
    the staged chain never touches it).  expect = the row asked for the persistent kernel and has its geometry: it must have
    stamped frame 0, with no failure counted; any other row must not have stamped."""

    def __init__(self, expect):
        self.expect = bool(expect)

    def __enter__(self):
        from flowtron_amd import _lib as L
        from flowtron_amd import ops
        dev = torch.device("cuda", 0)
        if self.expect:
            assert ops.persist_usable(dev), "an earlier persistent launch of this process failed: the device was switched to the staged kernels"
        self.before = _failures()
        self.prof = torch.zeros(512, 12, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        L.check(L.lib().ft_decode_debug_prof(L.ptr(self.prof)), "ft_decode_debug_prof")
        return self

    def __exit__(self, et, ev, tb):
        from flowtron_amd import _lib as L
        from flowtron_amd import ops
        torch.cuda.synchronize()
        L.lib().ft_decode_debug_prof(None)
        if et is not None:
            return False
        stamped = bool(self.prof[0].any().item())
        assert _failures() == self.before, "a persistent launch did not complete and the library decoded again on the staged kernels"
        assert ops.check_persist_status(raise_on_failure=False), "a persistent launch left its status word set"
        if self.expect:
            assert ops.persist_usable(torch.device("cuda", 0)), "the persistent kernels were switched off during this row"
            assert stamped, "this row asked for the persistent kernel and has its geometry, but the kernel left no stage stamps"
        else:
            assert not stamped, "a persistent kernel ran in a row that must decode on the staged chain"
        return False


_STEPS = {}


def flow_setup(small, over, gate):
    """(cfg, w = the last flow's weights on the CPU, AR_Step on the device), cached.  Without `gate` the flow has no gate layer."""
    from flowtron_amd import model as Mdl
    from oracle import flowtron_oracle as O
    key = (small, over, gate)
    if key not in _STEPS:
        cfg, sd = R.model_sd(small=small, **dict(over))
        w = R.flow_weights(sd, O.flow_prefix(cfg["n_flows"] - 1))
        if not gate:
            w = {k: v for k, v in w.items() if not k.startswith("gate_layer.")}
        M, S, C = cfg["n_mel_channels"], cfg["n_speaker_dim"], cfg["n_text_dim"]
        step = Mdl.AR_Step(M, S, C, M + S, cfg["n_hidden"], cfg["n_attn_channels"], cfg["n_lstm_layers"], gate, cfg["use_cumm_attention"])
        step.load_state_dict(w, strict=True)
        _STEPS[key] = (cfg, w, step.cuda().eval())
    return _STEPS[key]


def project(step, enc_dev, mode):
    """K, V as AR_Step.infer computes them in this operand mode (flowtron_amd.decode.infer: its two ops.linear calls)"""
    from flowtron_amd import ops
    att = step.attention_layer
    with env(FLOWTRON_MFMA=mode):
        t = enc_dev[:, None, :].contiguous()
        A = att.key.linear_layer.weight.shape[0]
        return (ops.linear(t, att.key.linear_layer.weight, None).reshape(-1, A).clone(),
                ops.linear(t, att.value.linear_layer.weight, None).reshape(-1, A).clone())


_REF = {}


def reference(key, w, residual, K, V, **kw):
    """(ref, D_mel, D_attn) of this case on these K, V: cached per key while the kernel's K, V and the residual stay bit-identical.
    The weights and keyword arguments are NOT compared: the key must imply them.  It does -- (case name, operand mode[, utterance
    or flow]) fixes the configuration, the rounding and, for a gated case, the gate designed for that mode."""
    K, V = K.cpu(), V.cpu()
    hit = _REF.get(key)
    if hit is not None and torch.equal(hit[0], K) and torch.equal(hit[1], V) and torch.equal(hit[2], residual):
        return hit[3]
    d_mel, d_attn, ref = R.deviation(w, residual, K, V, **kw)
    _REF[key] = (K, V, residual.clone(), (ref, d_mel, d_attn))
    return _REF[key][3]


U = 2.0 ** -24          # fp32 unit roundoff


def rowsum_bound(Lk):
    """|sum_l attn[l] - 1| of a correct fp32 softmax, first order, from the kernels' code.  Every decoder normalises alike
    (dec_ctx_k softmax_inplace, decode.hip:258-274; dec_persist_k :642-651; dec_persist_batch_k likewise): p_l = fl(e_l / s) with
    s the fp32 sum of the SAME e_l -- a thread adds ceil(L / 256) terms, a wave reduces in 6 steps, 4 wave partials take 3 adds.
    Errors of the e_l themselves cancel in sum_l e_l / s; what remains is s's summation error, at most (ceil(L/256) + 6 + 3) U
    relative, plus one division rounding U per element, weighted by p_l (sum 1).  The element tolerance 10 x D_attn cannot serve
    here: D_attn is 5e-10 .. 2e-8, below the rounding of a sum near 1 (U = 6e-8).  Independent of the case's data; 6.6e-7 at
    L <= 256, 9e-7 at L = 1025.  Against the reference's own row sum (1 to 1e-16; a forced row's given sum, where the error is 0)."""
    return (-(-Lk // 256) + 6 + 3 + 1) * U


def report(capsys, dec_name, case_name, mel, attn, ref, d_mel, d_attn, floor, note=""):
    """prints max error / D, then asserts the bound, the row sums and the signs.  mel [n,M], attn [n,L] float32 CPU."""
    n, Lk = ref["n_done"], ref["attn"].shape[1]
    assert mel.shape == ref["mel"].shape and attn.shape == ref["attn"].shape, (mel.shape, ref["mel"].shape, attn.shape)
    assert torch.isfinite(mel).all() and torch.isfinite(attn).all()
    tol_mel, tol_attn = R.tolerance(d_mel, d_attn, floor if n <= 9 else None)
    e_mel = (mel.double() - ref["mel"]).abs().max().item()
    e_attn = (attn.double() - ref["attn"]).abs().max().item()
    r_mel = e_mel / (tol_mel / R.MARGIN) if tol_mel > 0 else (0.0 if e_mel == 0 else float("inf"))
    r_attn = e_attn / (tol_attn / R.MARGIN) if tol_attn > 0 else (0.0 if e_attn == 0 else float("inf"))
    ds = (attn.double().sum(1) - ref["attn"].sum(1)).abs().max().item() if n else 0.0
    with capsys.disabled():
        print("\n[decode f64] %-22s | %-28s frames %3d | mel err %.2e D %.2e ratio %6.2f | attention err %.2e D %.2e ratio %6.2f | row sum err %.2e of %.2e %s"
              % (dec_name, case_name, n, e_mel, tol_mel / R.MARGIN, r_mel, e_attn, tol_attn / R.MARGIN, r_attn, ds, rowsum_bound(Lk), note), flush=True)
    wkey = dec_name + (" -> staged chain" if note else "")           # rows the library routed elsewhere are summarised apart
    wm, wa, ws = WORST.get(wkey, (0.0, 0.0, 0.0))
    WORST[wkey] = (max(wm, r_mel), max(wa, r_attn), max(ws, ds / rowsum_bound(Lk)))
    assert e_mel <= tol_mel, "mel: max error %.3e > 10 x D = %.3e (ratio to D %.1f)" % (e_mel, tol_mel, r_mel)
    assert e_attn <= tol_attn, "attention: max error %.3e > 10 x D = %.3e (ratio to D %.1f)" % (e_attn, tol_attn, r_attn)
    assert (attn >= 0).all()
    assert ds <= rowsum_bound(Lk), "attention row sums: %.3e > %.3e" % (ds, rowsum_bound(Lk))


def floor_of(key, w, K, V, cfg, sd_inputs, mode, **kw):
    """D of the ungated 17-frame decode of the same configuration (same text, keys, values, rounding)"""
    w0 = {k: v for k, v in w.items() if not k.startswith("gate_layer.")}
    _, d_mel, d_attn = reference(("floor",) + key, w0, sd_inputs, K, V, rounding=ROUNDING[mode], **kw)
    return d_mel, d_attn


def case_tensors(case, cfg):
    _, sd = R.model_sd(small=case.small, **dict(case.over))
    residual, enc = R.case_inputs(cfg, sd, max(case.N, 17), case.Lk)
    g = torch.Generator().manual_seed(5)
    prior = forced = None
    if case.prior:
        from oracle import flowtron_oracle as O
        prior = O.beta_binomial_prior(case.Lk, case.N).float()
    if case.forced:
        forced = torch.softmax(torch.randn(case.N, case.Lk, generator=g) * 2, 1)
    return residual[:case.N].contiguous(), residual[:17].contiguous(), enc, prior, forced


def run_case(case, dec, capsys):
    from flowtron_amd import ops
    dev = torch.device("cuda", 0)
    gated = case.stop != "nogate"
    cfg, w, step = flow_setup(case.small, case.over, gated)
    takes = persistent_geometry(cfg, case.Lk, case)
    if dec.persist and takes:
        need_persist(dec)
    residual, res17, enc, prior, forced = case_tensors(case, cfg)
    rounding = ROUNDING[dec.mode]
    cumm = cfg["use_cumm_attention"]
    kw = dict(temperature=case.temperature)
    if cumm:
        kw["enc"] = enc
    enc_dev = enc.to(dev)
    if gated:                                   # the gate layer, designed from the float64 trajectory of this rounding
        K0, V0 = project(step, enc_dev, dec.mode)
        free = R.decode({k: v for k, v in w.items() if not k.startswith("gate_layer.")}, residual, K0, V0, rounding=rounding, **kw)
        gw, gb = R.design_gate([free["gate_in"]], [case.stop])
        w = dict(w, **{"gate_layer.linear_layer.weight": gw, "gate_layer.linear_layer.bias": gb})
        with torch.no_grad():
            step.gate_layer.linear_layer.weight.copy_(gw)
            step.gate_layer.linear_layer.bias.copy_(gb)
        step.gate_threshold = 0.5
        kw["gate_threshold"] = 0.5
    step.attention_layer.temperature = case.temperature
    r_dev = residual.to(dev)[:, None, :].contiguous()
    t_dev = enc_dev[:, None, :].contiguous()
    ikw = dict(attns=None if forced is None else forced.to(dev), attn_prior=None if prior is None else prior.to(dev)[None],
               use_graph=dec.graph)
    with dec_env(dec):
        with Watch(dec.persist and takes):
            step.infer(r_dev, t_dev, **ikw)                     # allocates this shape's buffers
        bufs = step._decode_bufs[(case.N, case.Lk, str(r_dev.device))]
        bufs["mel"].fill_(SENT)
        with Watch(dec.persist and takes):
            mel, rows = step.infer(r_dev, t_dev, **ikw)
    K, V = bufs["K"].clone(), bufs["V"].clone()
    raw_mel, raw_attn = bufs["mel"].cpu(), bufs["attn"].cpu()
    key = (case.name, dec.mode)
    ref, d_mel, d_attn = reference(key, w, residual, K, V, rounding=rounding, prior=prior, forced=forced, **kw)
    n = ref["n_done"]
    if gated:
        margin = (ref["gate_logit"] - R.logit_threshold(0.5)).abs().min().item()
        assert margin >= 0.5, "the designed gate leaves only %.3f between a logit and the threshold" % margin
        assert n == (case.N if case.stop is None else case.stop + 1)
    assert mel.shape[0] == n and len(rows) == n, "frames produced: kernel %d, reference %d" % (mel.shape[0], n)
    if gated:
        assert int(bufs["n_done"].item()) == n
    floor = floor_of(key, w, K, V, cfg, res17, dec.mode, **{k: v for k, v in kw.items() if k != "gate_threshold"}) if n <= 9 else None
    attn = torch.cat([r.reshape(1, -1) for r in rows]).cpu() if n else torch.zeros(0, case.Lk)
    note = "(routed to the staged chain)" if dec.persist and not takes else ""
    report(capsys, dec.name, case.name, mel[:, 0].cpu(), attn, ref, d_mel, d_attn, floor, note)
    # rows past the stop: mel_out is not written, attn_out keeps infer()'s zeros
    assert torch.equal(raw_mel[:n], mel[:, 0].cpu())
    assert (raw_mel[n:] == SENT).all(), "mel_out rows past the stop were written"
    assert not raw_attn[n:].any(), "attn_out rows past the stop were written"


@pytest.mark.parametrize("dec", DECODERS, ids=lambda d: d.name.replace(" ", "_").replace(",", ""))
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_single_utterance_vs_float64(case, dec, capsys):
    run_case(case, dec, capsys)


@pytest.mark.parametrize("dec", F16_DECODERS, ids=lambda d: d.name.replace(" ", "_"))
def test_f16_operand_mode_decodes_from_the_bf16_images(dec, capsys):
    """FT_F16: model.py hands ft_decode_flow the same wimg scratch, and decode.hip has one image format -- bf16.  The reference
    with bf16 rounding must therefore hold at the full-width bench shape (the key / value projections, which do run with fp16
    operands, are inputs here)."""
    run_case(CASES[0]._replace(name="bench shape, FT_F16"), dec, capsys)


# ---------------------------------------------------------------------------------------------------- f32_to_bf16_k bit for bit
def test_weight_images_equal_torch_bf16_cast_bit_for_bit_ties_included():
    """the ten images ft_decode_flow leaves in wimg == torch's .to(bfloat16) of the ten matrices, in make_wimg's order and 256-byte
    packing.  attention_lstm.weight_ih_l0 carries every tie pattern: low half 0x8000 under an even and under an odd bf16
    significand (round to even goes down / up), one above and one below the tie, both signs, several exponents."""
    from flowtron_amd import model as Mdl
    cfg, sd = R.model_sd(small=True)
    from oracle import flowtron_oracle as O
    w = {k: v.clone() for k, v in R.flow_weights(sd, O.flow_prefix(1)).items() if not k.startswith("gate_layer.")}
    hi = torch.tensor([0x3F80, 0x3F81, 0xBF80, 0xBF81, 0x3C00, 0x3C7F, 0x4049, 0xC0FF, 0x3EFF, 0x3E00], dtype=torch.int64)
    lo = torch.tensor([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0xC000, 0x4000], dtype=torch.int64)
    bits = ((hi[:, None] << 16) | lo[None, :]).reshape(-1)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    special = bits.view(torch.float32)
    assert torch.isfinite(special).all() and special.abs().max() < 8
    wa = w["attention_lstm.weight_ih_l0"]
    wa.view(-1)[: special.numel()] = special
    wa.view(-1)[-special.numel():] = special.flip(0)
    M, S, C = cfg["n_mel_channels"], cfg["n_speaker_dim"], cfg["n_text_dim"]
    H, A = cfg["n_hidden"], cfg["n_attn_channels"]
    step = Mdl.AR_Step(M, S, C, M + S, H, A, 2, False, False)
    step.load_state_dict(w, strict=True)
    step = step.cuda().eval()
    residual, enc = R.case_inputs(cfg, sd, 2, 5)
    with dec_env(DECODERS[3]):
        step.infer(residual.cuda()[:, None, :].contiguous(), enc.cuda()[:, None, :].contiguous())
    torch.cuda.synchronize()
    img = step._decode_wimg.cpu()
    off, ties = 0, 0
    for k in R.ROUNDED:
        src = w[k].reshape(-1)
        nb = src.numel() * 2
        got = img[off:off + nb].view(torch.int16)
        want = src.to(torch.bfloat16).view(torch.int16)
        assert torch.equal(got, want), (k, int((got != want).sum()))
        ties += int(((src.view(torch.int32) & 0xFFFF) == 0x8000).sum())
        off += (nb + 255) & ~255
    assert off == img.numel() and ties >= 2 * len(hi)


# ---------------------------------------------------------------------------------------------------------------- batched launches
BatchCase = namedtuple("BatchCase", "name in_lens out_lens stops", defaults=(None,))
BATCH_CASES = [
    BatchCase("batch of 2", [21, 21], [17, 17]),
    BatchCase("batch of 3", [21, 33, 9], [17, 11, 14]),
    BatchCase("batch of 4 (one full group)", [21] * 4, [17, 12, 17, 9]),
    BatchCase("batch of 5 (group of 4 + group of one)", [21] * 5, [17, 12, 17, 9, 14]),
    BatchCase("batch of 5, stops at different frames", [21] * 5, [24, 17, 24, 9, 20], [3, None, 11, 0, 7]),
    BatchCase("ragged batch, text 1 .. 1000", [1000, 1, 513, 130, 57], [12, 17, 9, 14, 11]),
    BatchCase("ragged batch with stops", [157, 2, 64, 1000, 65], [17, 17, 12, 14, 17], [None, 5, 11, 2, 16]),
]
BATCH_DECODERS = [Decoder("f32 batched persistent", "f32", 1, True), Decoder("bf16 batched persistent", "bf16", 1, True)]


@pytest.mark.parametrize("dec", BATCH_DECODERS, ids=lambda d: d.name.replace(" ", "_"))
@pytest.mark.parametrize("bc", BATCH_CASES, ids=lambda c: c.name.replace(" ", "_").replace(",", ""))
def test_batched_launch_vs_float64(bc, dec, capsys):
    """AR_Step.infer_batch: groups of up to ft_decode_batch_max() utterances in one launch (ft_decode_flow_batch; with texts of
    different lengths ft_decode_flow_batch_keys), a trailing group of one on ft_decode_flow.  Every utterance against its own
    float64 decode on its own K, V rows."""
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    need_persist(dec)
    dev = torch.device("cuda", 0)
    gated = bc.stops is not None
    cfg, w, step = flow_setup(False, (), gated)
    _, sd = R.model_sd()
    B, Lmax, Nmax = len(bc.in_lens), max(bc.in_lens), max(bc.out_lens)
    assert L.lib().ft_decode_batch_max() == 4 and persistent_geometry(cfg, Lmax)
    rounding = ROUNDING[dec.mode]
    res, encs = [], []
    for b in range(B):
        r, e = R.case_inputs(cfg, sd, max(bc.out_lens[b], 17), bc.in_lens[b], seed=500 + 10 * b)
        res.append(r)
        encs.append(e)
    x = torch.zeros(Nmax, B, cfg["n_mel_channels"])
    text = torch.zeros(Lmax, B, encs[0].shape[1])
    for b in range(B):
        x[:bc.out_lens[b], b] = res[b][:bc.out_lens[b]]
        x[bc.out_lens[b]:, b] = float("nan")                   # frames behind an utterance's length are never read
        text[:bc.in_lens[b], b] = encs[b]
        text[bc.in_lens[b]:, b] = float("nan")                 # nor text positions behind its length
    x, text = x.to(dev), text.to(dev)
    KV = [project(step, encs[b].to(dev), dec.mode) for b in range(B)]
    if gated:
        w0 = {k: v for k, v in w.items() if not k.startswith("gate_layer.")}
        free = [R.decode(w0, res[b][:bc.out_lens[b]], KV[b][0], KV[b][1], rounding=rounding)["gate_in"] for b in range(B)]
        gw, gb = R.design_gate(free, bc.stops)
        w = dict(w, **{"gate_layer.linear_layer.weight": gw, "gate_layer.linear_layer.bias": gb})
        with torch.no_grad():
            step.gate_layer.linear_layer.weight.copy_(gw)
            step.gate_layer.linear_layer.bias.copy_(gb)
        step.gate_threshold = 0.5
    step.attention_layer.temperature = 1.0
    with dec_env(dec):
        with Watch(True):
            out, attn, n = step.infer_batch(x, text, list(bc.out_lens), list(bc.in_lens))
    # the one batched group's own K, V buffers == the projections used here
    kb = step._decode_batch_bufs[(min(B, 4), max(bc.out_lens[:4]), Lmax, str(dev))]
    for j in range(min(B, 4)):
        assert torch.equal(kb["K"][j, :bc.in_lens[j]], KV[j][0]) and torch.equal(kb["V"][j, :bc.in_lens[j]], KV[j][1]), j
    out, attn = out.cpu(), attn.cpu()
    assert tuple(attn.shape[1:]) == (B, 1, Lmax)
    for b in range(B):
        nb, lb = bc.out_lens[b], bc.in_lens[b]
        kw = dict(gate_threshold=0.5) if gated else {}
        ref, d_mel, d_attn = reference((bc.name, dec.mode, b), w, res[b][:nb], KV[b][0], KV[b][1], rounding=rounding, **kw)
        if gated:
            margin = (ref["gate_logit"] - R.logit_threshold(0.5)).abs().min().item()
            assert margin >= 0.5, margin
            assert ref["n_done"] == (nb if bc.stops[b] is None else bc.stops[b] + 1)
        assert int(n[b]) == ref["n_done"], (b, n, ref["n_done"])
        nd = ref["n_done"]
        floor = floor_of((bc.name, dec.mode, b), w, KV[b][0], KV[b][1], cfg, res[b][:17], dec.mode) if nd <= 9 else None
        report(capsys, dec.name, "%s [%d: L %d]" % (bc.name, b, lb), out[:nd, b], attn[:nd, b, 0, :lb], ref, d_mel, d_attn, floor)
        assert not out[nd:, b].any(), "mel rows behind utterance %d's end" % b
        assert not attn[nd:, b].any(), "attention rows behind utterance %d's end" % b
        assert not attn[:, b, 0, lb:].any(), "attention columns behind utterance %d's keys" % b


# ------------------------------------------------------------------------------------------------- the 2-flow model, flow by flow
@pytest.mark.parametrize("dec", DECODERS, ids=lambda d: d.name.replace(" ", "_").replace(",", ""))
def test_two_flow_model_flow_by_flow(dec, capsys):
    """Flowtron.infer at the shape bench.py times (2 flows, 69 symbols, 400 frames, sigma 0.5).  Each flow's AR_Step.infer is
    recorded: its residual (what the previous flow's kernel produced, flipped by AR_Back_Step for the odd flow), the encoder
    output the GPU computed, its K / V buffers and its output; the float64 reference decodes each flow from exactly those."""
    import flowtron
    from flowtron_amd import ops
    from oracle import flowtron_oracle as O
    need_persist(dec)
    cfg, sd = R.model_sd()
    N, Lk = 400, 69
    rs = np.random.RandomState(404)
    residual = torch.from_numpy(rs.standard_normal((1, 80, N)).astype(np.float32)) * 0.5
    txt = torch.from_numpy(rs.randint(0, cfg["n_text"], (1, Lk)))
    key = "two-flow model"
    if key not in _STEPS:
        m = flowtron.Flowtron(**cfg)
        m.load_state_dict(sd)
        _STEPS[key] = m.cuda().eval()
    m = _STEPS[key]
    rec = []
    steps = [f.ar_step if hasattr(f, "ar_step") else f for f in m.flows]

    def recorder(i, st, orig):
        def infer(res_in, text, *a, **k):
            o = orig(res_in, text, *a, **k)
            b = st._decode_bufs[(res_in.shape[0], text.shape[0], str(res_in.device))]
            rec.append((i, res_in[:, 0].cpu(), text[:, 0].cpu(), b["K"].clone(), b["V"].clone(), o[0][:, 0].cpu(),
                        torch.cat([r.reshape(1, -1) for r in o[1]]).cpu()))
            return o
        return infer

    try:
        for i, st in enumerate(steps):
            st.infer = recorder(i, st, st.infer)
        with dec_env(dec):
            with Watch(dec.persist):
                mel, _ = m.infer(residual.cuda(), torch.zeros(1, dtype=torch.long).cuda(), txt.cuda(), gate_threshold=2.0)
    finally:
        for st in steps:
            del st.infer
    assert [r[0] for r in rec] == [1, 0] and mel.shape == (1, 80, N)
    assert torch.equal(rec[0][1], torch.flip(residual[0].t(), (0,)))            # the odd flow decodes the reversed residual
    assert torch.equal(rec[1][1], torch.flip(rec[0][5], (0,)))                  # and hands its frames back in natural order
    assert torch.equal(mel[0].t().cpu(), rec[1][5])
    for i, res_in, enc, K, V, out, attn in rec:
        w = R.flow_weights(sd, O.flow_prefix(i))
        ref, d_mel, d_attn = reference(("two-flow", i, dec.mode), w, res_in, K, V, rounding=ROUNDING[dec.mode], gate_threshold=2.0)
        report(capsys, dec.name, "2-flow model, flow %d" % i, out, attn, ref, d_mel, d_attn, None)


def test_zz_worst_ratio_per_decoder(capsys):
    with capsys.disabled():
        print("\n[decode f64] worst max error / D per decoder (bound: %g)" % R.MARGIN)
        for k, (rm, ra, rs) in WORST.items():
            print("   %-42s mel %6.2f   attention %6.2f   row sum error / its bound %5.2f" % (k, rm, ra, rs))
