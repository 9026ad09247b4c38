"""Golden vectors for the style-transfer posterior: the REAL reference notebook's own cell (inference_style_transfer.ipynb,
the code cell under "Compute the posterior distribution") executed on CPU over given z_values.

Run once in the build container:   python tests/golden/make_golden_style.py   ->   tests/golden/style_posterior.pt

The notebook is read from the reference checkout at generation time and the cell's text is executed from there as it is; only
its three assignment lines `lambd = ...`, `n_frames = ...` and `aggregation_type = ...` are substituted.  Stored: the inputs
(each utterance's z [80, len]) and the cell's `mu_posterior` per case, keyed "<aggregation>/<n_frames>".

  exact    4 utterances of 8, 16, 32 and 4 frames, entries k / 16 with integer k in -8 .. 8, lambd = 4 (ratio = 1, c = 0.5),
           n_frames 1, 20, 50, both aggregations: every fp32 operation of the notebook is exact, so its result is THE answer
  random   N(0, 1) utterances of 37, 1, 20, 36 and 7 frames, lambd = 1e-4, n_frames = 100, both aggregations; `dev64` records
           the notebook's deviation from the float64 restatement (tests/style_ref64.py)
"""
import json
import os
import re
import sys

import numpy as np
import torch
from torch.distributions import Normal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import style_ref64 as R  # noqa: E402
from oracle import refshim  # noqa: E402

CELL = 14          # nbformat index of the cell that assigns aggregation_type and forms mu_posterior
M = 80


def notebook_cell():
    with open(os.path.join(refshim.REF_DIR, "inference_style_transfer.ipynb")) as f:
        cell = json.load(f)["cells"][CELL]
    src = "".join(cell["source"])
    assert cell["cell_type"] == "code" and "aggregation_type" in src and "mu_posterior" in src, "the notebook's layout changed"
    return src


def run_cell(src, zs, lambd, n_frames, aggregation):
    """-> the cell's mu_posterior over z_values = [z[None] for z in zs] (CPU fp32 [1, 80, len], as cell 12 leaves them)"""
    for name, value in (("lambd", repr(lambd)), ("n_frames", repr(n_frames)), ("aggregation_type", repr(aggregation))):
        src, n = re.subn(r"(?m)^%s = .*$" % name, "%s = %s" % (name, value), src)
        assert n == 1, name
    env = {"torch": torch, "Normal": Normal, "z_values": [z[None].clone() for z in zs], "print": lambda *a: None}
    exec(compile(src, "inference_style_transfer.ipynb#cell%d" % CELL, "exec"), env)
    return env["mu_posterior"].clone()


def main():
    assert refshim.available(), "needs the reference checkout"
    src = notebook_cell()
    res = {}

    rs = np.random.RandomState(21)
    zs = [torch.from_numpy((rs.randint(-8, 9, size=(M, n)) / 16.0).astype(np.float32)) for n in (8, 16, 32, 4)]
    case = {"z": zs, "lambd": 4.0, "mu": {}}
    for agg in ("batch", "time_and_batch"):
        for nf in (1, 20, 50):
            mu = run_cell(src, zs, 4.0, nf, agg)
            ref, _ = R.posterior_mean([z.numpy() for z in zs], 4.0, agg, nf)
            assert mu.dtype == torch.float32 and np.array_equal(mu.numpy().astype(np.float64), ref), (agg, nf)
            case["mu"]["%s/%d" % (agg, nf)] = mu
    res["exact"] = case

    rs = np.random.RandomState(22)
    zs = [torch.from_numpy(rs.standard_normal((M, n)).astype(np.float32)) for n in (37, 1, 20, 36, 7)]
    case = {"z": zs, "lambd": 1e-4, "mu": {}, "dev64": {}}
    for agg in ("batch", "time_and_batch"):
        mu = run_cell(src, zs, 1e-4, 100, agg)
        ref, S = R.posterior_mean([z.numpy() for z in zs], 1e-4, agg, 100)
        err = np.abs(mu.numpy().astype(np.float64) - ref)
        assert (err <= R.notebook_bound(S, len(zs), agg, 37)).all(), agg
        case["mu"]["%s/100" % agg] = mu
        case["dev64"][agg] = float(err.max())
    res["random"] = case

    path = os.path.join(HERE, "style_posterior.pt")
    torch.save(res, path)
    print("style_posterior.pt", os.path.getsize(path) // 1024, "KiB", "dev64", {k: "%.2e" % v for k, v in case["dev64"].items()})


if __name__ == "__main__":
    main()
