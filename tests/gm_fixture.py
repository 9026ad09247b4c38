"""Shared between tests/golden/make_golden_gm.py (which runs the real reference) and the mixture tests (which read gm_small.pt): the
cases, the seeded weights of the 20 state_dict entries the mixture adds, and how a gradient is stored (not collected by pytest).

gm_small.pt stores no weights but the fixed Gaussians' buffers (the reference's constructor draws them): the base model's come from
oracle/synth.make_state_dict and the mixture's from mixture_weights below, both by seed; the fixture carries the reference's key order and
shapes, which the rebuilt state_dict must reproduce.  Gradients of up to FULL_GRAD elements are stored whole; a larger one as every
GRAD_STRIDE-th element of the flattened tensor plus the float64 norm of the whole (three whole sets of this model's gradients would not
fit the size limit of a committed fixture)."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import synth

FULL_GRAD, GRAD_STRIDE = 1024, 8

CASES = OrderedDict([
    ("fixed", dict(cfg=dict(n_components=4, fixed_gaussian=True, mean_scale=3.0), out_lens=[9, 5, 7], in_lens=[4, 3, 3], seed=21)),
    ("learned", dict(cfg=dict(n_components=3, fixed_gaussian=False, mean_scale=0.0), out_lens=[9, 5, 7], in_lens=[4, 3, 3], seed=22)),
    ("learned1", dict(cfg=dict(n_components=3, fixed_gaussian=False, mean_scale=0.0), out_lens=[9], in_lens=[4], seed=22)),
])
BUFFERS = ("gaussian_mixture.mean", "gaussian_mixture.log_var")


def model_config(name):
    return dict(synth.SMALL_MODEL_CONFIG, mel_encoder_n_hidden=64, **CASES[name]["cfg"])


def mixture_weights(spec, base_sd, seed, buffers):
    """spec: [(key, shape)] in the reference's order.  The base model's entries from base_sd, the fixed Gaussians from `buffers`, the
    rest random and well conditioned: component means spread over the range of z, log-variances around 0.5."""
    rs = np.random.RandomState(seed + 100)
    sd = OrderedDict()
    for k, shp in spec:
        shp = tuple(shp)
        if k in base_sd:
            sd[k] = base_sd[k]
            continue
        if k in BUFFERS:
            sd[k] = buffers[k].clone()
            continue
        if ".1.weight" in k:
            w = 1.0 + 0.1 * rs.standard_normal(shp)
        elif k.endswith("bias"):
            w = 0.05 * rs.standard_normal(shp)
            if "mean_layer" in k:
                w = 2.0 * rs.standard_normal(shp) - 4.0
            if "log_var_layer" in k:
                w = 0.5 * rs.standard_normal(shp) + 0.5
        else:
            w = rs.uniform(-1.0, 1.0, shp) / np.sqrt(int(np.prod(shp[1:])))
            if "gaussian_mixture" in k:
                w = w * 4.0
        sd[k] = torch.from_numpy(np.ascontiguousarray(w)).float()
    return sd


def state_dict_of(name, case):
    """the state_dict of fixture case `case` (gm_small.pt[name]), rebuilt"""
    cfg = model_config(name)
    seed = CASES[name]["seed"]
    return mixture_weights(case["spec"], synth.make_state_dict(cfg, seed=seed), seed, case["buffers"])


def batch_of(name):
    c = CASES[name]
    return synth.make_batch(model_config(name), c["out_lens"], c["in_lens"], seed=c["seed"], with_prior=True)


def pack_grad(g):
    g = g.detach()
    if g.numel() <= FULL_GRAD:
        return {"full": g.clone()}
    return {"sample": g.reshape(-1)[::GRAD_STRIDE].clone(), "norm": float(g.double().norm())}


def grad_view(packed, g):
    """(reference values, the matching view of gradient g, the reference's whole-tensor norm | None)"""
    if "full" in packed:
        return packed["full"], g, None
    return packed["sample"], g.reshape(-1)[::GRAD_STRIDE], packed["norm"]
