"""Golden vectors of the Gaussian-mixture prior (flowtron.py:217-231, 312-450, 846-851, 877-881): the REAL reference on CPU through
oracle/refshim.py -> tests/golden/gm_small.pt.  Run once in the build container:   python tests/golden/make_golden_gm.py

Base config: synth.SMALL_MODEL_CONFIG with mel_encoder_n_hidden = 64, 2 flows, coupling convolutions randomised (synth.make_state_dict),
train mode, gm_loss with the gate and CTC terms on.  Cases:
  fixed     fixed_gaussian, C 4, mean_scale 3, B 3, out_lens [9, 5, 7] (not sorted), in_lens [4, 3, 3]
  learned   learned mean and variance, C 3 (not a power of two), the same batch
  learned1  `learned` at B 1 (the unmasked instance norm, flowtron.py:417)
Per case: the state_dict's key order and shapes and the fixed Gaussians' buffers (every other weight and the inputs are rebuilt by seed:
tests/gm_fixture.py, oracle/synth.py), the dropout keep-masks, the forward's 8-tuple, the three losses and every parameter gradient of
nll + gate + 0.01 ctc (large ones sampled, gm_fixture.pack_grad).

Dropout: F.dropout is replaced by a multiplication with GIVEN keep-masks (values 0 or 2), in call order: the text encoder's three
convolutions, then the mel encoder's two.  An identity stub would not do: the mel encoder zero-fills its input in place (:420), which
would hit the ReLU output autograd still needs, and the reference's own backward raises."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import refshim, synth  # noqa: E402
import gm_fixture as GF  # noqa: E402


def run_case(R, name):
    spec, cfg = GF.CASES[name], GF.model_config(name)
    seed, out_lens, in_lens = spec["seed"], spec["out_lens"], spec["in_lens"]
    np.random.seed(seed)                                       # GaussianMixture.generate_mean draws with np.random.choice
    m = R.Flowtron(**cfg)
    key_spec = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    buffers = {k: v.clone() for k, v in m.state_dict().items() if k in GF.BUFFERS}
    sd = GF.mixture_weights(key_spec, synth.make_state_dict(cfg, seed=seed), seed, buffers)
    m.load_state_dict(sd)
    b = GF.batch_of(name)
    B, T, Lt = len(out_lens), max(out_lens), max(in_lens)
    g = torch.Generator().manual_seed(seed)
    masks = [torch.bernoulli(torch.full((B, cfg["n_text_dim"], Lt), 0.5), generator=g) * 2.0 for _ in range(3)]
    masks += [torch.bernoulli(torch.full((B, cfg["mel_encoder_n_hidden"], T), 0.5), generator=g) * 2.0 for _ in range(2)]
    queue = list(masks)
    crit = R.FlowtronLoss(1.0, True, True, True, 0.01, -8)
    real_dropout = F.dropout
    F.dropout = lambda x, p=0.5, training=True, inplace=False: x * queue.pop(0)
    try:
        m.train()
        out = m(b["mel"].clone(), b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"], b["attn_prior"].clone())
        snap_lp = [x.detach().clone() for x in out[4]]         # the loss rolls the odd flows' log-probabilities in place
        nll, gl, ctc = crit(out, b["gate_target"], b["in_lens"], b["out_lens"])
        (nll + gl + 0.01 * ctc).backward()
    finally:
        F.dropout = real_dropout
    assert not queue
    z, log_s, gate, attn, _, mean, log_var, prob = out
    return {"cfg": cfg, "spec": key_spec, "buffers": buffers, "keep_masks": [k.to(torch.uint8) for k in masks],
            "out": {"z": z.detach(), "log_s": [x.detach().clone() for x in log_s], "gate": gate.detach(), "attn": [x.detach() for x in attn],
                    "logprob": snap_lp, "mean": mean.detach(), "log_var": log_var.detach(), "prob": prob.detach()},
            "nll": nll.detach(), "gate_loss": gl.detach(), "ctc": ctc.detach(),
            "grads": OrderedDict((k, GF.pack_grad(p.grad)) for k, p in m.named_parameters())}


def main():
    assert refshim.available(), "needs the reference checkout"
    torch.set_num_threads(4)
    R = refshim.load()
    res = OrderedDict((name, run_case(R, name)) for name in GF.CASES)
    path = os.path.join(HERE, "gm_small.pt")
    torch.save(res, path)
    print("gm_small.pt", os.path.getsize(path), "bytes; small_f3.pt", os.path.getsize(os.path.join(HERE, "small_f3.pt")), "bytes")
    for name, r in res.items():
        print(name, "nll %.6f gate %.6f ctc %.6f" % (r["nll"].item(), r["gate_loss"].item(), r["ctc"].item()),
              "prob", r["out"]["prob"][0].tolist())


if __name__ == "__main__":
    main()
