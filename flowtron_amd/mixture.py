"""Gaussian-mixture prior at inference time.  The reference trains the mixture (flowtron.py:217-231, 312-450) but has no inference
use of it; the paper samples z from ONE component to pick a speaking style.  Two steps:

    mean, log_var, prob = mixture_parameters(model, mel, out_lens)      # what the mel encoder makes of reference utterances
    z = sample_component(mean, log_var, component=2, n_frames=300, sigma=0.5)
    mel_out, attn = model.infer(z, speaker_ids, text)

Everything runs on the device (csrc/mixture.hip); there is no CPU path.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import ops
from .model import lengths_arg


def mixture_parameters(model, mel, out_lens):
    """The mixture a model built with n_components > 1 assigns to a batch of utterances, without gradients and without running the
    flows: mel [B, M, T] (not modified), out_lens [B] (list or integer tensor, 1 ..= T), utterances in any order ->
    (mean, log_var, prob) = ([B or 1, M, C], [B or 1, M, C], [B, C]); one row for the fixed Gaussians.  Dropout follows
    model.training: call model.eval() for a deterministic result.  The pooled embedding divides by the LONGEST length of the batch
    (flowtron.py:437-439), so an utterance's parameters depend on the batch it comes in, as they do in training."""
    if not hasattr(model, "gaussian_mixture"):
        raise ValueError("the model has no mixture: it was built with n_components <= 1")
    L.require_cuda(mel)
    if mel.dim() != 3:
        raise ValueError("mel must be [B, M, T], got %s" % (tuple(mel.shape),))
    ol = lengths_arg(out_lens, "out_lens", mel.shape[0], mel.shape[2])
    if ol is None:
        raise ValueError("out_lens must be given")
    with torch.no_grad():
        lens = torch.tensor(ol, dtype=torch.int32, device=mel.device)
        e = model.mel_encoder(mel, lens)
        mean, log_var, prob = model.gaussian_mixture(e, e.size(0))
        return mean.detach().clone(), log_var.detach().clone(), prob


def sample_component(mean, log_var, component, n_frames, sigma=1.0, rows=None, generator=None):
    """z ~ N(mean_k, sigma^2 exp(log_var_k)) frame by frame, ready for model.infer: mean, log_var [Bm, M, C] as mixture_parameters
    returns them; component: an int or a list of S ints in 0 .. C-1 (one sample each); rows: which row of mean / log_var each
    sample takes (int or list of S; None = row 0 for Bm 1, row s for sample s otherwise) -> fp32 [S, M, n_frames].
    sigma = 0 returns the component means exactly.  generator: a torch.Generator of mean's device for the N(0, 1) draws."""
    L.require_cuda(mean, log_var)
    if mean.dim() != 3 or mean.shape != log_var.shape:
        raise ValueError("mean and log_var must both be [Bm, M, C], got %s and %s" % (tuple(mean.shape), tuple(log_var.shape)))
    Bm, M, Cn = mean.shape
    comp = [component] if isinstance(component, int) else list(component)
    S = len(comp)
    if S < 1 or any(isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < Cn for k in comp):
        raise ValueError("component must hold integers in 0 ..= %d, got %r" % (Cn - 1, component))
    if rows is None:
        if Bm != 1 and S != Bm:
            raise ValueError("rows must be given: %d samples from %d rows of mean / log_var" % (S, Bm))
        row = [0] * S if Bm == 1 else list(range(S))
    else:
        row = [rows] * S if isinstance(rows, int) else list(rows)
    if len(row) != S or any(isinstance(r, bool) or not isinstance(r, int) or not 0 <= r < Bm for r in row):
        raise ValueError("rows must hold %d integers in 0 ..= %d, got %r" % (S, Bm - 1, rows))
    if int(n_frames) < 1 or float(sigma) < 0.0:
        raise ValueError("n_frames must be >= 1 and sigma >= 0")
    dev = mean.device
    eps = None
    if float(sigma) > 0.0:
        eps = torch.randn(S, M, int(n_frames), device=dev, dtype=torch.float32, generator=generator)
    return ops.mixture_sample(mean, log_var, torch.tensor(comp, dtype=torch.int32, device=dev), int(n_frames), float(sigma),
                              torch.tensor(row, dtype=torch.int32, device=dev), eps)
