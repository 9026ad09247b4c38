"""tests/decode_ref64.py is right, and sharp (no GPU).

Right: with rounding=None it agrees with oracle.ar_step_infer run in float64 to float64 rounding, on every branch the GPU
test uses.  The oracle is pinned to the real reference by the goldens (tests/test_oracle_golden.py), so this ties the new
reference to the real one.

Sharp: at the bench shape (full-width last flow of the 2-flow model, 69 text symbols, 400 frames) a decode that leaves ONE of
the ten rounded matrices unrounded, reads a stale h of the top decoder layer, or shifts one attention row by one text position
must differ from the fully rounded reference by at least 10 x the GPU test's tolerance (decode_ref64.MARGIN x D) on mel or on
attention.  Float64 against float64, so it runs anywhere.  Measured with GAIN = 3, as mutation / (MARGIN x D), mel | attention
(D = 2.0e-7 mel, 8.0e-9 attention on this case; |mel| <= 2.2, nothing saturates):
    attention_lstm.weight_ih_l0   27.9 | 18.9        lstm.weight_hh_l1            37.4 |  0.6
    attention_lstm.weight_hh_l0   14.4 |  8.1        dense_layer.layers.0 weight  31.8 |  0.4
    attention query weight         0.0 | 12.2        dense_layer.layers.1 weight  41.5 |  0.4
    lstm.weight_ih_l0             45.8 |  0.5        conv.weight                  40.3 |  0.5
    lstm.weight_hh_l0             47.7 |  0.6        stale h of decoder layer 1   3502 | 34.3
    lstm.weight_ih_l1             34.4 |  0.5        attention row 200 shifted     9.5 | 119966
So attention has to be compared as well as mel (the query weight shows on attention alone).  The test prints the measured
ratios and asserts that each mutation reaches 10 on mel or on attention."""
import os

import pytest
import torch

import decode_ref64 as R
from oracle import flowtron_oracle as O

F64_TOL = 1e-11          # float64 rounding through <= 24 frames of values of order 1 (observed: ~1e-14)


def small_case(N=12, Lk=9, gate=False, **over):
    cfg, sd = R.model_sd(small=True, seed=31, **over)
    pfx = O.flow_prefix(cfg["n_flows"] - 1)
    w = R.flow_weights(sd, pfx)
    if not gate:
        w = {k: v for k, v in w.items() if not k.startswith("gate_layer.")}
    residual, enc = R.case_inputs(cfg, sd, N, Lk, seed=7)
    K = enc @ w["attention_layer.key.linear_layer.weight"].t()
    V = enc @ w["attention_layer.value.linear_layer.weight"].t()
    return w, residual, K, V, enc


def agree(w, residual, K, V, **kw):
    ref = R.decode(w, residual, K, V, **kw)
    o = R.oracle_decode(w, residual, K, V, dtype=torch.float64, **kw)
    assert o["n_done"] == ref["n_done"]
    assert o["mel"].dtype == torch.float64
    dm = (o["mel"] - ref["mel"]).abs().max().item()
    da = (o["attn"] - ref["attn"]).abs().max().item()
    assert dm <= F64_TOL and da <= F64_TOL, (dm, da)
    return ref, o


@pytest.mark.parametrize("N,Lk", [(12, 9), (1, 9), (12, 1), (24, 40)])
def test_plain_agrees_with_float64_oracle(N, Lk):
    agree(*small_case(N, Lk)[:4])


def test_temperature():
    w, r, K, V, _ = small_case()
    ref, _ = agree(w, r, K, V, temperature=0.7)
    assert (ref["attn"] - R.decode(w, r, K, V)["attn"]).abs().max() > 1e-4


@pytest.mark.parametrize("depth", [1, 3])
def test_depth(depth):
    w, r, K, V, _ = small_case(n_lstm_layers=depth)
    assert ("lstm.weight_ih_l2" in w) == (depth == 3) and ("lstm.weight_ih_l1" in w) == (depth == 3)
    agree(w, r, K, V)


def test_cumulative_attention():
    w, r, K, V, enc = small_case(use_cumm_attention=True)
    ref, _ = agree(w, r, None, V, enc=enc)
    plain = {k: v for k, v in w.items() if not k.startswith("attn_cond_layer.")}
    assert (ref["attn"] - R.decode(plain, r, K, V)["attn"]).abs().max() > 1e-4      # the location layer does something


def test_prior_rows():
    w, r, K, V, _ = small_case()
    prior = O.beta_binomial_prior(9, 12).float()               # exact in fp32, as the kernel receives it
    ref, _ = agree(w, r, K, V, prior=prior)
    assert (ref["attn"] - R.decode(w, r, K, V)["attn"]).abs().max() > 1e-3


def test_forced_alignment():
    w, r, K, V, _ = small_case()
    forced = torch.softmax(torch.randn(12, 9, generator=torch.Generator().manual_seed(1)) * 2, 1)
    ref, _ = agree(w, r, K, V, forced=forced)
    assert torch.equal(ref["attn"], forced.double())


@pytest.mark.parametrize("stop", [0, 5, 11, None])
def test_gate_designed_from_the_trajectory(stop):
    w, r, K, V, _ = small_case(gate=True)
    free = R.decode({k: v for k, v in w.items() if not k.startswith("gate_layer.")}, r, K, V)
    gw, gb = R.design_gate([free["gate_in"]], [stop])
    w = dict(w, **{"gate_layer.linear_layer.weight": gw, "gate_layer.linear_layer.bias": gb})
    ref, o = agree(w, r, K, V, gate_threshold=0.5)
    assert ref["n_done"] == (12 if stop is None else stop + 1)
    thr = R.logit_threshold(0.5)
    assert (ref["gate_logit"] - thr).abs().min() >= 0.5
    assert (o["gate_logit"] - ref["gate_logit"]).abs().max() < 1e-9
    assert torch.equal(ref["mel"], free["mel"][: ref["n_done"]])


def test_oracle_sd_hands_the_oracle_exactly_these_keys_and_values():
    """the identity projection is exact in fp32: perturbing K in its last bit moves the oracle's fp32 output"""
    w, r, K, V, _ = small_case()
    a = R.oracle_decode(w, r, K, V)
    K2 = K.clone()
    K2.view(torch.int32)[:] += 1
    b = R.oracle_decode(w, r, K2, V)
    sd, encp = R.oracle_sd(w, K, V)
    assert torch.equal(encp[:, 0] @ sd["f.attention_layer.key.linear_layer.weight"].t(), K)
    assert torch.equal(encp[:, 0] @ sd["f.attention_layer.value.linear_layer.weight"].t(), V)
    assert not torch.equal(a["attn"], b["attn"])


def test_deviation_helper_and_tolerance_rule():
    w, r, K, V, _ = small_case(N=17)
    d_mel, d_attn, ref = R.deviation(w, r, K, V, rounding=torch.bfloat16)
    assert 0 < d_mel < 1e-5 and 0 < d_attn < 1e-6                  # fp32 arithmetic noise, not weight rounding
    d1 = R.deviation(w, r[:1], K, V, rounding=torch.bfloat16)
    assert R.tolerance(d1[0], d1[1], floor=(d_mel, d_attn)) == (R.MARGIN * max(d1[0], d_mel), R.MARGIN * max(d1[1], d_attn))
    assert R.tolerance(d_mel, d_attn) == (R.MARGIN * d_mel, R.MARGIN * d_attn)
    # rounding is what separates the modes: far above the noise
    unr = R.decode(w, r, K, V)
    assert (unr["mel"] - ref["mel"]).abs().max() > 100 * d_mel


def test_rounding_touches_exactly_the_ten_matrices():
    w = small_case(gate=True, use_cumm_attention=True)[0]
    rw = R.round_weights(w, torch.bfloat16)
    changed = sorted(k for k in w if not torch.equal(rw[k], w[k]))
    assert changed == sorted(R.ROUNDED)
    w3 = small_case(n_lstm_layers=3)[0]
    rw3 = R.round_weights(w3, torch.bfloat16)
    assert torch.equal(rw3["lstm.weight_ih_l2"], w3["lstm.weight_ih_l2"]) and torch.equal(rw3["lstm.weight_hh_l2"], w3["lstm.weight_hh_l2"])


SHARPNESS = {}


def test_sharpness_one_mutation_per_rounded_matrix(capsys):
    """bench shape, GAIN = 3.  Prints mutation / (MARGIN x D) on mel and on attention; each mutation must reach 10 on one of them."""
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    cfg, sd = R.model_sd()
    pfx = O.flow_prefix(cfg["n_flows"] - 1)
    w = {k: v for k, v in R.flow_weights(sd, pfx).items() if not k.startswith("gate_layer.")}
    residual, enc = R.case_inputs(cfg, sd, 400, 69)
    K = enc @ w["attention_layer.key.linear_layer.weight"].t()
    V = enc @ w["attention_layer.value.linear_layer.weight"].t()
    bf = torch.bfloat16
    d_mel, d_attn, ref = R.deviation(w, residual, K, V, rounding=bf)
    tol_mel, tol_attn = R.tolerance(d_mel, d_attn)
    muts = [(k, dict(keep=(k,))) for k in R.ROUNDED] + [("stale h of decoder layer 1", dict(stale_h1=True)),
                                                         ("attention row 200 shifted by one", dict(shift_frame=200))]
    rows = []
    for name, kw in muts:
        m = R.decode(w, residual, K, V, rounding=bf, **kw)
        rm = (m["mel"] - ref["mel"]).abs().max().item() / tol_mel
        ra = (m["attn"] - ref["attn"]).abs().max().item() / tol_attn
        rows.append((name, rm, ra))
        SHARPNESS[name] = (rm, ra)
    with capsys.disabled():
        print("\n[decode_ref64 sharpness] bench shape, gain %g: D mel %.2e attention %.2e, |mel| <= %.2f" % (R.GAIN, d_mel, d_attn, ref["mel"].abs().max()))
        for name, rm, ra in rows:
            print("   %-48s mutation / (10 D): mel %8.1f   attention %8.1f" % (name, rm, ra))
    assert ref["mel"].abs().max() < 10 and torch.isfinite(ref["mel"]).all()
    bad = [r for r in rows if max(r[1], r[2]) < 10.0]
    assert not bad, bad
