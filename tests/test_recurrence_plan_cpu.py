"""The decisions of the recurrence dispatch in flowtron_amd.ops that are pure functions of plain values, held against tables written out
by hand -- no device, no library, no stubs.

* ops.decoder_plan: which branch of model.AR_Step.forward runs the decoder LSTM stack, and whether the gate layer rides on layer 0's
  input projection.  PLAN is what AR_Step.forward decided before the plan existed (its `persist` / `fuse_gate` expressions and its
  if / elif chain over n_lstm_layers, persist, rowmap, decoder_pair_chunks, lstm2_supported), row by row.
* ops._dgates_exit: how layer-0 dgates leave a persistent backward.  Before the rule existed LSTMSeqFn.backward and the decoder pair
  each spelled it out; both spellings are transcribed below and must agree with each other and with EXIT on all twelve rows.
* ops._persist_env: the one reader of FLOWTRON_LSTM_PERSIST.
"""
import pytest
import torch

from flowtron_amd import ops

# n_layers  gate  rowmap  persistent  pair_chunks  lstm2_ok  ->  path  fuse_gate
PLAN = """
1 0 0 0 0 0 layers 0
1 0 0 0 0 1 layers 0
1 0 0 0 6 0 layers 0
1 0 0 0 6 1 layers 0
1 0 0 1 0 0 layers 0
1 0 0 1 0 1 layers 0
1 0 0 1 6 0 layers 0
1 0 0 1 6 1 layers 0
1 0 1 0 0 0 layers 0
1 0 1 0 0 1 layers 0
1 0 1 0 6 0 layers 0
1 0 1 0 6 1 layers 0
1 0 1 1 0 0 layers 0
1 0 1 1 0 1 layers 0
1 0 1 1 6 0 layers 0
1 0 1 1 6 1 layers 0
1 1 0 0 0 0 layers 1
1 1 0 0 0 1 layers 1
1 1 0 0 6 0 layers 1
1 1 0 0 6 1 layers 1
1 1 0 1 0 0 layers 1
1 1 0 1 0 1 layers 1
1 1 0 1 6 0 layers 1
1 1 0 1 6 1 layers 1
1 1 1 0 0 0 layers 1
1 1 1 0 0 1 layers 1
1 1 1 0 6 0 layers 1
1 1 1 0 6 1 layers 1
1 1 1 1 0 0 layers 1
1 1 1 1 0 1 layers 1
1 1 1 1 6 0 layers 1
1 1 1 1 6 1 layers 1
2 0 0 0 0 0 step 0
2 0 0 0 0 1 lstm2 0
2 0 0 0 6 0 step 0
2 0 0 0 6 1 lstm2 0
2 0 0 1 0 0 persistent 0
2 0 0 1 0 1 persistent 0
2 0 0 1 6 0 persistent 0
2 0 0 1 6 1 persistent 0
2 0 1 0 0 0 step 0
2 0 1 0 0 1 lstm2 0
2 0 1 0 6 0 step 0
2 0 1 0 6 1 lstm2 0
2 0 1 1 0 0 persistent 0
2 0 1 1 0 1 persistent 0
2 0 1 1 6 0 pair 0
2 0 1 1 6 1 pair 0
2 1 0 0 0 0 step 1
2 1 0 0 0 1 lstm2 0
2 1 0 0 6 0 step 1
2 1 0 0 6 1 lstm2 0
2 1 0 1 0 0 persistent 1
2 1 0 1 0 1 persistent 1
2 1 0 1 6 0 persistent 1
2 1 0 1 6 1 persistent 1
2 1 1 0 0 0 step 1
2 1 1 0 0 1 lstm2 0
2 1 1 0 6 0 step 1
2 1 1 0 6 1 lstm2 0
2 1 1 1 0 0 persistent 1
2 1 1 1 0 1 persistent 1
2 1 1 1 6 0 pair 1
2 1 1 1 6 1 pair 1
3 0 0 0 0 0 layers 0
3 0 0 0 0 1 layers 0
3 0 0 0 6 0 layers 0
3 0 0 0 6 1 layers 0
3 0 0 1 0 0 layers 0
3 0 0 1 0 1 layers 0
3 0 0 1 6 0 layers 0
3 0 0 1 6 1 layers 0
3 0 1 0 0 0 layers 0
3 0 1 0 0 1 layers 0
3 0 1 0 6 0 layers 0
3 0 1 0 6 1 layers 0
3 0 1 1 0 0 layers 0
3 0 1 1 0 1 layers 0
3 0 1 1 6 0 layers 0
3 0 1 1 6 1 layers 0
3 1 0 0 0 0 layers 1
3 1 0 0 0 1 layers 1
3 1 0 0 6 0 layers 1
3 1 0 0 6 1 layers 1
3 1 0 1 0 0 layers 1
3 1 0 1 0 1 layers 1
3 1 0 1 6 0 layers 1
3 1 0 1 6 1 layers 1
3 1 1 0 0 0 layers 1
3 1 1 0 0 1 layers 1
3 1 1 0 6 0 layers 1
3 1 1 0 6 1 layers 1
3 1 1 1 0 0 layers 1
3 1 1 1 0 1 layers 1
3 1 1 1 6 0 layers 1
3 1 1 1 6 1 layers 1
"""


def _plan_rows():
    rows = [line.split() for line in PLAN.strip().splitlines()]
    return [(int(r[0]), bool(int(r[1])), bool(int(r[2])), bool(int(r[3])), int(r[4]), bool(int(r[5])), r[6], bool(int(r[7]))) for r in rows]


def test_decoder_plan_table_is_complete():
    keys = {r[:6] for r in _plan_rows()}
    want = {(n, g, rm, p, c, l2) for n in (1, 2, 3) for g in (False, True) for rm in (False, True) for p in (False, True) for c in (0, 6)
            for l2 in (False, True)}
    assert keys == want and len(_plan_rows()) == 96


@pytest.mark.parametrize("row", _plan_rows(), ids=lambda r: "n%d-g%d-rm%d-p%d-c%d-l%d" % tuple(int(v) for v in r[:6]))
def test_decoder_plan(row):
    n, gate, rowmap, persistent, chunks, lstm2_ok, path, fuse_gate = row
    got = ops.decoder_plan(n, gate, rowmap, persistent, chunks, lstm2_ok)
    assert got == (path, fuse_gate)
    assert type(got[1]) is bool


# FLOWTRON_LSTM_PERSIST_IMG, anomaly mode, gx_private  ->  (hand_image, keep_f32)
EXIT = [
    ("0", False, False, (False, True)),
    ("0", False, True, (False, True)),
    ("0", True, False, (False, True)),
    ("0", True, True, (False, True)),
    ("1", False, False, (False, True)),
    ("1", False, True, (True, False)),       # the training step: the image is the ONLY form
    ("1", True, False, (False, True)),
    ("1", True, True, (True, True)),         # anomaly mode inspects what the node returns: real values beside the image
    ("both", False, False, (True, True)),
    ("both", False, True, (True, True)),
    ("both", True, False, (True, True)),
    ("both", True, True, (True, True)),
]


def _exit_lstm_seq(img, anomaly, private):
    """LSTMSeqFn.backward as it was: the recurrence emits (and hands over) the image where `_PERSIST_IMG != "0" and (gx_private or
    _PERSIST_IMG == "both")`; then `img_only = _PERSIST_IMG != "both" and not anomaly`, and fp32 rows unless img_only"""
    hand = img != "0" and (private or img == "both")
    img_only = hand and img != "both" and not anomaly
    return hand, not img_only


def _exit_pair(img, anomaly, private):
    """the decoder pair as it was: keep_f32 in DecoderPairFn.backward, hand in _pair_backward_return"""
    keep_f32 = img != "1" or anomaly or not private
    hand = img != "0" and (private or img == "both")
    return hand, keep_f32


@pytest.mark.parametrize("img,anomaly,private,want", EXIT)
def test_dgates_exit(monkeypatch, img, anomaly, private, want):
    assert _exit_lstm_seq(img, anomaly, private) == want
    assert _exit_pair(img, anomaly, private) == want
    monkeypatch.setattr(ops, "_PERSIST_IMG", img)
    with torch.autograd.set_detect_anomaly(anomaly):
        assert torch.is_anomaly_enabled() == anomaly
        got = ops._dgates_exit(private)
    assert got == want
    assert not (not got[0] and not got[1]), "dgates must leave in some form"


def test_dgates_exit_table_is_complete():
    assert {r[:3] for r in EXIT} == {(i, a, p) for i in ("0", "1", "both") for a in (False, True) for p in (False, True)}


def test_persist_env(monkeypatch):
    monkeypatch.setenv("FLOWTRON_LSTM_PERSIST", "0")
    assert ops._persist_env() == 0
    monkeypatch.setenv("FLOWTRON_LSTM_PERSIST", "1")
    assert ops._persist_env() == 1
    monkeypatch.delenv("FLOWTRON_LSTM_PERSIST")
    assert ops._persist_env() == 1
    monkeypatch.setenv("FLOWTRON_LSTM_PERSIST", "2")
    with pytest.raises(ValueError):
        ops._persist_env()
