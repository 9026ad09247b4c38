"""Float64 restatement of one flow's autoregressive decode at the AR_Step.infer / ft_decode_flow boundary, with the decode
kernels' own operand rounding (imported by the tests, not collected).  Plain torch on the CPU; nothing here calls the
project's kernels, and nothing here calls the oracle except `deviation`, which measures the oracle against this module.

What the decode kernels round (csrc/decode.hip, decode_batch.hip, decode_persist.h, decode_dev.h; read on this revision):

  * fp32 weight mode (ft_decode_args.wimg NULL): nothing.  The staged chain streams the fp32 weights (dec_lstm_k, dec_gemv_k,
    dec_conv_k: decode.hip:107-162, :210-230, :356-364), dec_persist_k<true> keeps them in registers / LDS or streams them
    (decode.hip:439-447, :514-519) -- fp32 operands and fp32 FMAs everywhere.
  * 16-bit modes (wimg given; flowtron_amd.decode sets it for FT_BF16 AND FT_F16, `L.is16`, in infer and infer_batch): ftdec::make_wimg
    (decode.hip:864-881) rounds exactly TEN matrices with f32_to_bf16_k (decode.hip:775-780: pack_bf16x2 = the hardware's
    round-to-nearest-even convert, common.h:63-67), in this order:
        attention_lstm.weight_ih_l0, attention_lstm.weight_hh_l0, attention_layer.query weight,
        lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.weight_ih_l1, lstm.weight_hh_l1,
        dense_layer.layers.0 weight, dense_layer.layers.1 weight, conv.weight
    decode.hip is compiled once, for the bf16 format: FT_F16 mode decodes from the same bf16 images.
    The staged chain reads the images in dec_lstm16_k (decode.hip:167-206), dec_gemv_k (:224-225) and dec_conv_k (:361-362);
    dec_persist_k<false> and dec_persist_batch_k<false> load all ten into registers (decode.hip:508-527).  Activations and
    accumulation are fp32 in every mode.
  * Never rounded, in any mode and any of the three kernels families: v (decode.hip:242, :549), all biases (:141, :195, :533-536),
    K and V as the caller passes them (:239-242, :299, :547, :554, :628, :662), the gate weight and bias (:377-378, :391, :550,
    :555), the residual, prior and forced rows, the cumulative-attention convolutions, w_key and enc (dec_cond_k, dec_key_k:
    :308-353, staged chain only), and decoder layers beyond the second (enqueue_frame nulls their image slots, decode.hip:813-819;
    depth 1 copies layer 0's recurrent matrix into the unused layer-1 slots, :869-871).

So `rounding=torch.bfloat16` casts the ten matrices of ROUNDED with torch's `.to(torch.bfloat16)` (round to nearest even) and
keeps everything else; `rounding=None` keeps everything.  tests/test_gpu_decode_f64.py checks f32_to_bf16_k's images against that
cast bit for bit, ties included.

K and V are INPUTS: the key / value projections are GEMMs with their own tests, and a decode test must not inherit their
rounding of the text.  The gate LOGIT is returned for every frame, so a test can tell a stop decision within rounding of the
threshold from a wrong one.

The model of the full-width cases: synth.DEFAULT_MODEL_CONFIG, seed 23, with the six LSTM weight matrices of every flow
(attention_lstm and lstm layers 0 / 1, weight_ih and weight_hh) multiplied by GAIN = 3.  With the synthetic weights as they are,
leaving ONE of the recurrent matrices unrounded moves the output by about as much as the tolerance of the GPU test (the
recurrences are too weakly coupled to see it); with the gain every one of the ten moves it by more than ten times that
tolerance (tests/test_decode_ref64_cpu.py measures and asserts the ten ratios, and lists them)."""
import math

import torch
import torch.nn.functional as F

ROUNDED = (
    "attention_lstm.weight_ih_l0", "attention_lstm.weight_hh_l0", "attention_layer.query.linear_layer.weight",
    "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.weight_ih_l1", "lstm.weight_hh_l1",
    "dense_layer.layers.0.linear_layer.weight", "dense_layer.layers.1.linear_layer.weight", "conv.weight",
)
GAINED = ("attention_lstm.weight_ih_l0", "attention_lstm.weight_hh_l0", "lstm.weight_ih_l0", "lstm.weight_hh_l0",
          "lstm.weight_ih_l1", "lstm.weight_hh_l1")
GAIN = 3.0
MARGIN = 10.0            # the kernels are held to MARGIN x D (see tolerance)
_COND = "attn_cond_layer.location_conv_hidden.conv.weight"
_GATE = "gate_layer.linear_layer.weight"


def flow_weights(sd, pfx):
    """the tensors of one flow, keys without the flow's prefix"""
    return {k[len(pfx):]: v for k, v in sd.items() if k.startswith(pfx)}


def apply_gain(sd, gain=GAIN):
    """the six LSTM weight matrices of every flow times `gain`, in place (keys with or without a flow prefix)"""
    for k in sd:
        if any(k == g or k.endswith("." + g) for g in GAINED):
            sd[k] = sd[k] * gain
    return sd


def round_weights(w, rounding, keep=()):
    """fp32 tensors as the kernels of that mode read them: the ten matrices of ROUNDED cast to `rounding` and back (None: as they
    are); `keep` names matrices left unrounded (the sharpness mutations)."""
    out = {}
    for k, v in w.items():
        v = v.detach().float().cpu()
        if rounding is not None and k in ROUNDED and k not in keep:
            v = v.to(rounding).float()
        out[k] = v
    return out


def _cell(x, h, c, w_ih, w_hh, b):
    a = w_ih @ x + w_hh @ h + b
    i, f, g, o = a.chunk(4)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def decode(w, residual, K=None, V=None, *, enc=None, temperature=1.0, gate_threshold=0.5, prior=None, forced=None,
           rounding=None, keep=(), stale_h1=False, shift_frame=None):
    """One flow, float64.  w: flow_weights(); residual [N,M]; K, V [L,A] as the kernel received them; with cumulative attention
    (w holds the attn_cond_layer) enc [L,E] and w's key weight replace K (ft_decode_args: "K is then ignored"); prior / forced
    [N,L] rows or None.  The decoder depth is the number of lstm.weight_ih_l* in w; a gate layer in w switches the stop on.
    Returns dict(mel [N',M], attn [N',L], gate_logit [N'] (NaN without a gate), gate_in [N',H+A] = the rows [h_att ; ctx] the gate
    layer reads, n_done = N').
    Mutations (tests of the tests): keep = matrices left unrounded; stale_h1: the dense layer reads the last decoder layer's h
    of the PREVIOUS frame; shift_frame: that frame's attention row is rotated by one text position."""
    f64 = torch.float64
    p = {k: v.to(f64) for k, v in round_weights(w, rounding, keep).items()}
    res = residual.detach().cpu().to(f64)
    N, M = res.shape
    V = V.detach().cpu().to(f64)
    Lk, A = V.shape
    H = p["attention_lstm.weight_hh_l0"].shape[1]
    cumm = _COND in p
    if cumm:
        encd = enc.detach().cpu().to(f64)
        w_key = p["attention_layer.key.linear_layer.weight"]
        c1w, c1b = p[_COND], p["attn_cond_layer.location_conv_hidden.conv.bias"]
        c2w, c2b = p["attn_cond_layer.location_conv_out.conv.weight"], p["attn_cond_layer.location_conv_out.conv.bias"]
        cum_a, prev_a = torch.zeros(Lk, dtype=f64), torch.zeros(Lk, dtype=f64)
    else:
        Kd = K.detach().cpu().to(f64)
    if prior is not None:
        prior = prior.detach().cpu().to(f64).reshape(-1, Lk)
    if forced is not None:
        forced = forced.detach().cpu().to(f64).reshape(-1, Lk)
    n_layers = 0
    while "lstm.weight_ih_l%d" % n_layers in p:
        n_layers += 1
    v = p["attention_layer.v.linear_layer.weight"].reshape(-1)
    wq = p["attention_layer.query.linear_layer.weight"]
    b_att = p["attention_lstm.bias_ih_l0"] + p["attention_lstm.bias_hh_l0"]
    b_l = [p["lstm.bias_ih_l%d" % k] + p["lstm.bias_hh_l%d" % k] for k in range(n_layers)]
    conv_w = p["conv.weight"].reshape(2 * M, H)
    has_gate = _GATE in p
    z = lambda n: torch.zeros(n, dtype=f64)
    ha, ca = z(H), z(H)
    hs, cs = [z(H) for _ in range(n_layers)], [z(H) for _ in range(n_layers)]
    prev = z(M)
    mel, attn, logits, gin = [], [], [], []
    for i in range(N):
        ha, ca = _cell(prev, ha, ca, p["attention_lstm.weight_ih_l0"], p["attention_lstm.weight_hh_l0"], b_att)
        if forced is not None:
            a = forced[i]
        else:
            q = wq @ ha
            if cumm:                # Conv1d(2->32, k5) + ReLU, Conv1d(32->E, k3) + sigmoid over [cumulative ; previous] attention
                x = torch.stack([cum_a, prev_a])[None]
                x = torch.relu(F.conv1d(x, c1w, c1b, padding=2))
                cond = torch.sigmoid(F.conv1d(x, c2w, c2b, padding=1))[0].t()          # [L,E]
                Kd = (encd * cond) @ w_key.t()
            e = torch.tanh(q[None, :] + Kd) @ v / temperature
            a = torch.softmax(e, 0)
            if prior is not None:
                a = torch.softmax(torch.log(a + 1e-20) + torch.log(prior[i] + 1e-20), 0)
        if shift_frame is not None and i == shift_frame:
            a = torch.roll(a, 1)
        if cumm:
            prev_a = a
            cum_a = cum_a + a
        ctx = a @ V
        d = torch.cat([ha, ctx])
        u = d
        h_top_before = hs[-1]
        for k in range(n_layers):
            hs[k], cs[k] = _cell(u, hs[k], cs[k], p["lstm.weight_ih_l%d" % k], p["lstm.weight_hh_l%d" % k], b_l[k])
            u = hs[k]
        if stale_h1:
            u = h_top_before
        for j in range(2):
            u = torch.tanh(p["dense_layer.layers.%d.linear_layer.weight" % j] @ u + p["dense_layer.layers.%d.linear_layer.bias" % j])
        o = conv_w @ u + p["conv.bias"]
        prev = (res[i] - o[M:]) / torch.exp(o[:M])
        mel.append(prev)
        attn.append(a)
        gin.append(d)
        if has_gate:
            g = p[_GATE].reshape(-1) @ d + p["gate_layer.linear_layer.bias"][0]
            logits.append(g)
            if float(torch.sigmoid(g)) > gate_threshold:
                break
        else:
            logits.append(torch.tensor(float("nan"), dtype=f64))
    n = len(mel)
    return dict(mel=torch.stack(mel) if n else res.new_zeros(0, M), attn=torch.stack(attn) if n else res.new_zeros(0, Lk),
                gate_logit=torch.stack(logits) if n else res.new_zeros(0), gate_in=torch.stack(gin) if n else res.new_zeros(0, H + A),
                n_done=n)


def logit_threshold(gate_threshold):
    """the gate logit at which sigmoid = gate_threshold (inf: never stops, -inf: always)"""
    if gate_threshold >= 1.0:
        return math.inf
    if gate_threshold <= 0.0:
        return -math.inf
    return math.log(gate_threshold / (1.0 - gate_threshold))


def design_gate(gate_inputs, stops, margin=1.0):
    """Gate weights from float64 trajectories, as the 400-frame decode test designs them: the minimum-norm weight (bias 0) whose
    logit is -margin on every frame before an utterance's stop and +margin on the stop frame.  gate_inputs: per utterance the
    [n, H + A] rows [h_att ; ctx]; stops: per utterance the stop frame or None (never).  Returns weight [1, H + A], bias [1]."""
    rows, y = [], []
    for d, s in zip(gate_inputs, stops):
        n = d.shape[0] if s is None else s + 1
        rows.append(d[:n].double())
        t = -margin * torch.ones(n, dtype=torch.float64)
        if s is not None:
            t[s] = margin
        y.append(t)
    wgt = torch.linalg.pinv(torch.cat(rows)) @ torch.cat(y)
    return wgt.float().reshape(1, -1), torch.zeros(1)


# ------------------------------------------------------------------------------------------------------------ the oracle's own noise
def oracle_sd(w, K, V, rounding=None, enc=None, pfx="f."):
    """A state dict for oracle.ar_step_infer that makes it decode from EXACTLY these K and V.  The oracle projects its `enc`
    argument itself, so it is handed enc' = [K | V] (cumulative attention: [enc | V]) with the key weight [I | 0] ([w_key | 0])
    and the value weight [0 | I]: a product with one 1 and zeros is exact in any summation order and any precision.  The
    location layer's second convolution gets zero rows for the appended channels (their modulation multiplies zero key-weight
    columns).  Returns (sd, enc' [L,1,*])."""
    p = round_weights(w, rounding)
    V = V.detach().cpu().float()
    Lk, A = V.shape
    eye, zero = torch.eye(A), torch.zeros(A, A)
    sd = {pfx + k: t for k, t in p.items()}
    if _COND in p:
        e = enc.detach().cpu().float()
        E = e.shape[1]
        sd[pfx + "attention_layer.key.linear_layer.weight"] = torch.cat([p["attention_layer.key.linear_layer.weight"], zero], 1)
        sd[pfx + "attention_layer.value.linear_layer.weight"] = torch.cat([torch.zeros(A, E), eye], 1)
        for nm in ("location_conv_out", "conv_layers.2"):
            k = pfx + "attn_cond_layer.%s.conv." % nm
            if k + "weight" in sd:
                sd[k + "weight"] = torch.cat([sd[k + "weight"], torch.zeros(A, 32, 3)], 0)
                sd[k + "bias"] = torch.cat([sd[k + "bias"], torch.zeros(A)], 0)
        encp = torch.cat([e, V], 1)
    else:
        sd[pfx + "attention_layer.key.linear_layer.weight"] = torch.cat([eye, zero], 1)
        sd[pfx + "attention_layer.value.linear_layer.weight"] = torch.cat([zero, eye], 1)
        encp = torch.cat([K.detach().cpu().float(), V], 1)
    return sd, encp[:, None, :]


class F64Prior:
    """The oracle reads a prior row as `attn_prior[:, i].float()`, which would evaluate its logarithm in fp32 even in a float64
    run.  This wrapper hands it the float64 rows unchanged, so a float64 run of the oracle is float64 throughout."""

    class _Row:
        def __init__(self, t):
            self.t = t

        def float(self):
            return self.t

    def __init__(self, t):
        self.t = t

    def __getitem__(self, idx):
        return F64Prior._Row(self.t[idx])


def oracle_decode(w, residual, K, V, *, dtype=torch.float32, rounding=None, enc=None, temperature=1.0, gate_threshold=0.5,
                  prior=None, forced=None):
    """oracle.ar_step_infer on the same rounded weights and the same K, V, computing in `dtype`.
    Returns dict(mel, attn, gate_logit, n_done) like `decode`."""
    from oracle import flowtron_oracle as O
    sd, encp = oracle_sd(w, K, V, rounding, enc)
    sd = {k: t.to(dtype) for k, t in sd.items()}
    has_gate = "f." + _GATE in sd
    gates = []
    pr = None
    if prior is not None:
        pr = prior.detach().cpu().reshape(1, -1, V.shape[0])
        pr = F64Prior(pr.double()) if dtype == torch.float64 else pr.float()
    fo = None if forced is None else forced.detach().cpu().to(dtype).reshape(-1, V.shape[0])
    with torch.no_grad():
        mel, attn = O.ar_step_infer(sd, "f.", residual.detach().cpu().to(dtype)[:, None, :], encp.to(dtype), has_gate,
                                    temperature, gate_threshold, pr, fo, gates if has_gate else None)
    n = mel.shape[0]
    gl = torch.logit(torch.tensor([g[0] for g in gates], dtype=torch.float64)) if has_gate else torch.full((n,), float("nan"), dtype=torch.float64)
    return dict(mel=mel[:, 0], attn=attn.reshape(n, -1), gate_logit=gl, n_done=n)


def deviation(w, residual, K, V, ref=None, **kw):
    """(D_mel, D_attn, ref): the largest deviation, over every element, of oracle.ar_step_infer IN FP32 ON THE CPU from this
    module's float64 decode, both on the same rounded weights and the same K, V -- the reference implementation's own
    arithmetic noise on the case.  kw as for `decode` (without the mutations).  Both must stop at the same frame."""
    if ref is None:
        ref = decode(w, residual, K, V, **kw)
    o = oracle_decode(w, residual, K, V, dtype=torch.float32, **kw)
    assert o["n_done"] == ref["n_done"], "the fp32 oracle stops at frame %d, the float64 reference at %d" % (o["n_done"], ref["n_done"])
    d_mel = (o["mel"].double() - ref["mel"]).abs().max().item()
    d_attn = (o["attn"].double() - ref["attn"]).abs().max().item()
    return d_mel, d_attn, ref


def tolerance(d_mel, d_attn, floor=None):
    """The bound of the GPU test: MARGIN x D on mel and on attention separately; `floor` = the (D_mel, D_attn) of the 17-frame case
    of the same configuration, taken where it is larger (cases of at most 9 frames: their own deviation is tiny and noisy)."""
    if floor is not None:
        d_mel, d_attn = max(d_mel, floor[0]), max(d_attn, floor[1])
    return MARGIN * d_mel, MARGIN * d_attn


# ------------------------------------------------------------------------------------------------------------ the test models
_SD = {}


def model_sd(small=False, gain=GAIN, seed=23, **over):
    """(cfg, state dict) of the synthetic 2-flow model with the LSTM gain applied (cached: tests must not modify it in place)"""
    from oracle import synth
    key = (small, gain, seed, tuple(sorted(over.items())))
    if key not in _SD:
        cfg = dict(synth.SMALL_MODEL_CONFIG if small else synth.DEFAULT_MODEL_CONFIG, **over)
        _SD[key] = (cfg, apply_gain(synth.make_state_dict(cfg, seed=seed), gain))
    return _SD[key]


def case_inputs(cfg, sd, N, Lk, seed=404, sigma=0.5):
    """residual [N,M] and the oracle encoder's output enc [L,E] (fp32, CPU) for a random text of Lk symbols.  Frame i of the
    residual does not depend on N (a shorter case is a prefix of a longer one)."""
    import numpy as np
    from oracle import flowtron_oracle as O
    rs = np.random.RandomState(seed)
    txt = torch.from_numpy(rs.randint(0, cfg["n_text"], (1, Lk)))
    residual = torch.from_numpy(np.random.RandomState(seed + 1).standard_normal((N, cfg["n_mel_channels"])).astype(np.float32)) * sigma
    with torch.no_grad():
        enc = O.embed_and_encode(sd, torch.zeros(1, dtype=torch.long), txt, None, cfg.get("dummy_speaker_embedding", False))
    return residual, enc[:, 0].contiguous()
