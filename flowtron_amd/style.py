"""Style transfer (the reference's inference_style_transfer.ipynb): the posterior over z given reference speech.

The notebook runs the model forward over a set of reference utterances, averages their latents z (`aggregation_type`
'batch': every z tiled along time to n_frames, mean over the utterances; 'time_and_batch': mean over time, then over the
utterances), shrinks the mean towards the prior N(0, 1) by ratio / (ratio + 1), ratio = K / lambd, and samples the z that
Flowtron.infer turns into speech in the reference's style.  Here the sums are kept on the device in a float64 accumulator
(csrc/style.hip) that batches of any size are added into, so a reference set larger than one batch is accumulated batch by
batch -- with the same bits however it is split -- and the samples are formed on the device as well:

    post = StylePosterior(aggregation="batch", n_frames=300)
    for mel, speaker_ids, text, in_lens, out_lens in reference_batches:
        post.add_utterances(model, mel, speaker_ids, text, in_lens, out_lens, force_speaker_id=0)
    mel, _ = model.infer(post.sample(sigma=1.0), speaker_id, text_encoded)

There is no CPU path: tensors on the host are refused.
"""
from __future__ import annotations

import numbers

import torch

from . import _lib as L
from . import ops
from .model import lengths_arg

AGGREGATIONS = {"batch": L.STYLE_BATCH, "time_and_batch": L.STYLE_TIME_AND_BATCH}


class StylePosterior:
    """Posterior over z from the latents of reference utterances (notebook cells `aggregation_type` / `dist.sample`).

    aggregation "batch" keeps a mean per (mel channel, frame) of the utterances tiled to n_frames (required: it fixes the
    accumulator's shape); "time_and_batch" keeps one mean per mel channel (n_frames is ignored).  lambd as in the notebook."""

    def __init__(self, n_mel_channels=80, aggregation="batch", n_frames=None, lambd=1e-4):
        if aggregation not in AGGREGATIONS:
            raise ValueError("aggregation must be 'batch' or 'time_and_batch', got %r" % (aggregation,))
        if isinstance(n_mel_channels, bool) or not isinstance(n_mel_channels, numbers.Integral) or n_mel_channels < 1:
            raise ValueError("n_mel_channels must be a positive integer, got %r" % (n_mel_channels,))
        if aggregation == "batch":
            if n_frames is None:
                raise ValueError("aggregation 'batch' needs n_frames: it fixes the shape of the posterior mean")
            if isinstance(n_frames, bool) or not isinstance(n_frames, numbers.Integral) or n_frames < 1:
                raise ValueError("n_frames must be a positive integer, got %r" % (n_frames,))
        if not float(lambd) > 0.0:
            raise ValueError("lambd must be positive, got %r" % (lambd,))
        self.n_mel_channels = int(n_mel_channels)
        self.aggregation = aggregation
        self.n_frames = int(n_frames) if aggregation == "batch" else None
        self.lambd = float(lambd)
        self.count = 0                 # utterances added so far (the notebook's len(z_values))
        self._mode = AGGREGATIONS[aggregation]
        self._acc = None               # float64 [M, n_frames] | [M, 1] on the device of the first z

    def add(self, z, lengths):
        """Adds the utterances of one batch: z [B, M, T] fp32 on the device, any strides (Flowtron.latents' output, or the
        forward's time-major [T, B, M] z as `.permute(1, 2, 0)`, is read in place); lengths [B]: the frames of each utterance,
        1 ..= T (a list, or an integer tensor on the host or the device).  Frames behind a length are never read."""
        if not torch.is_tensor(z) or z.dim() != 3:
            raise ValueError("z must be a [B, M, T] tensor, got %s" % (tuple(z.shape) if torch.is_tensor(z) else type(z).__name__,))
        B, M, T = z.shape
        if M != self.n_mel_channels:
            raise ValueError("z has %d mel channels, this posterior %d" % (M, self.n_mel_channels))
        if B < 1 or T < 1:
            raise ValueError("z must hold at least one utterance and one frame, got shape %s" % (tuple(z.shape),))
        if z.dtype != torch.float32:
            raise ValueError("z must be float32, got %s" % z.dtype)
        lens = lengths_arg(lengths, "lengths", B, T)
        if lens is None:
            raise ValueError("lengths must be given: the frames of every utterance")
        L.require_cuda(z)
        if self._acc is None:
            self._acc = torch.zeros(M, self.n_frames or 1, device=z.device, dtype=torch.float64)
        elif self._acc.device != z.device:
            raise ValueError("z is on %s, the utterances added before on %s" % (z.device, self._acc.device))
        lens32 = torch.tensor(lens, dtype=torch.int32, device=z.device)
        ops.style_accumulate(z.detach(), lens32, self._acc, self.n_frames or 1, self._mode)
        self.count += B
        return self

    def add_utterances(self, model, mel, speaker_ids, text, in_lens, out_lens, attn_prior=None, force_speaker_id=None):
        """Flowtron.latents of one batch of reference utterances followed by add(); returns their z [B, M, T].
        force_speaker_id: run every utterance as that speaker (the notebook's `sid * 0 + force_speaker_id`)."""
        if force_speaker_id is not None:
            speaker_ids = speaker_ids * 0 + force_speaker_id
        z = model.latents(mel, speaker_ids, text, in_lens, out_lens, attn_prior)
        self.add(z, out_lens)
        return z

    def _require_utterances(self):
        if self.count == 0:
            raise ValueError("no reference utterance has been added yet")

    def mean(self):
        """The notebook's mu_posterior: fp32 [M, n_frames] ('batch') or [M, 1] ('time_and_batch')."""
        self._require_utterances()
        return ops.style_sample(self._acc, self.count, self.lambd, self.n_mel_channels, self.n_frames or 1, self._mode)[0]

    def sample(self, n=1, sigma=1.0, n_frames=None, generator=None, eps=None):
        """n draws from N(mean, sigma^2) as fp32 [n, M, n_frames], the residual Flowtron.infer takes.  n_frames: the frames of a
        'time_and_batch' sample (required there: the one mean per channel is used at every frame); a 'batch' posterior has its
        own.  eps: the standard normal draws to use, fp32 [n, M, n_frames] on the device; otherwise torch.randn(..., generator=)."""
        self._require_utterances()
        if self.aggregation == "batch":
            if n_frames is not None:
                raise ValueError("a 'batch' posterior has n_frames = %d of its own" % self.n_frames)
            n_frames = self.n_frames
        elif n_frames is None or isinstance(n_frames, bool) or not isinstance(n_frames, numbers.Integral) or n_frames < 1:
            raise ValueError("a 'time_and_batch' sample needs n_frames, a positive integer; got %r" % (n_frames,))
        if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
            raise ValueError("n must be a positive integer, got %r" % (n,))
        shape = (int(n), self.n_mel_channels, int(n_frames))
        if eps is None:
            eps = torch.randn(shape, device=self._acc.device, dtype=torch.float32, generator=generator)
        else:
            if not torch.is_tensor(eps) or tuple(eps.shape) != shape or eps.dtype != torch.float32:
                raise ValueError("eps must be a float32 tensor of shape %s" % (shape,))
            L.require_cuda(eps)
            eps = eps.detach().contiguous()
        return ops.style_sample(self._acc, self.count, self.lambd, self.n_mel_channels, int(n_frames), self._mode, eps=eps,
                                sigma=float(sigma))
