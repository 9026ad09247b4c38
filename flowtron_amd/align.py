"""Token durations and pace control: from the model's attention to per-token durations, and from durations back to an
alignment that Flowtron.infer_aligned decodes along (additive: the reference has no alignment search).

    z, attn, logp = model.alignments(mel, speaker_ids, text, in_lens, out_lens)       # every flow in natural time
    path, durations = monotonic_alignment(logp[0], in_lens, out_lens)                 # frames per token (csrc/align.hip)
    durations, totals = scale_durations(durations, in_lens, pace=0.8)                 # slower speech: frames / 0.8
    rows = durations_to_alignment(durations, in_lens)                                 # hard [B, N, L] alignment
    mel, lengths = model.infer_aligned(residual, speaker_ids, text, rows, in_lens, n_frames=totals)

The search and the expansion run on the device and refuse tensors on the host; scale_durations is host arithmetic over the
B x L integers (the caller needs the totals on the host anyway, to allocate the residual)."""
from __future__ import annotations

import math
import numbers

import torch

from . import _lib as L
from . import ops
from .model import lengths_arg

MAX_TOKENS = 1024          # ft_mas_ragged: one thread per token, one workgroup per utterance


def monotonic_alignment(logp, in_lens, out_lens, return_score=False):
    """The best monotone path through logp [B, T, L] (fp32 on the device, any strides: a slice of Flowtron.alignments' or the
    forward's attn_logprob is read in place) for every utterance: it starts at token 0, ends at token in_lens[b] - 1 at frame
    out_lens[b] - 1, and moves on by 0 or 1 token per frame; among equally good paths the one that advances earliest.
    -> (path [B, T] int32, the token of every frame, -1 behind out_lens[b]; durations [B, L] int32, the frames of every token,
    >= 1 each, sum out_lens[b], 0 behind in_lens[b]) and, with return_score, score [B] fp32: the path's summed log-probability.
    in_lens / out_lens: lists, or integer tensors on the host or the device, 1 ..= L and 1 ..= T.  Scores behind the lengths are
    never read.  ValueError where an utterance has more tokens than frames; NotImplementedError for L > 1024."""
    if not torch.is_tensor(logp) or logp.dim() != 3:
        raise ValueError("logp must be a [B, T, L] tensor, got %s" % (tuple(logp.shape) if torch.is_tensor(logp) else type(logp).__name__,))
    B, T, Lt = logp.shape
    if B < 1 or T < 1 or Lt < 1:
        raise ValueError("logp must hold at least one utterance, frame and token, got shape %s" % (tuple(logp.shape),))
    if logp.dtype != torch.float32:
        raise ValueError("logp must be float32, got %s" % logp.dtype)
    il = lengths_arg(in_lens, "in_lens", B, Lt)
    ol = lengths_arg(out_lens, "out_lens", B, T)
    if il is None or ol is None:
        raise ValueError("in_lens and out_lens must be given")
    bad = [b for b in range(B) if il[b] > ol[b]]
    if bad:
        raise ValueError("utterance %d has in_lens %d > out_lens %d: no monotone alignment gives every token a frame"
                         % (bad[0], il[bad[0]], ol[bad[0]]))
    if Lt > MAX_TOKENS:
        raise NotImplementedError("monotonic_alignment holds at most %d tokens, got L = %d" % (MAX_TOKENS, Lt))
    L.require_cuda(logp)
    in32 = torch.tensor(il, dtype=torch.int32, device=logp.device)
    out32 = torch.tensor(ol, dtype=torch.int32, device=logp.device)
    path, dur, score = ops.mas_ragged(logp.detach(), in32, out32, want_score=return_score)
    return (path, dur, score) if return_score else (path, dur)


def _durations_arg(durations):
    if not torch.is_tensor(durations) or durations.dim() != 2:
        raise ValueError("durations must be a [B, L] tensor, got %s"
                         % (tuple(durations.shape) if torch.is_tensor(durations) else type(durations).__name__,))
    if durations.dtype.is_floating_point or durations.dtype.is_complex or durations.dtype == torch.bool:
        raise ValueError("durations must hold integers, got a %s tensor" % durations.dtype)
    if durations.shape[0] < 1 or durations.shape[1] < 1:
        raise ValueError("durations must hold at least one utterance and one token, got shape %s" % (tuple(durations.shape),))
    return durations.shape


def durations_to_alignment(durations, in_lens, n_frames=None, reverse=False):
    """durations [B, L] (integers on the device; negatives count as 0) -> the hard alignment [B, N, L] fp32: row n of
    utterance b is 1 at the token whose frames hold n, 0 elsewhere; rows at or behind the utterance's total and columns at or
    behind in_lens[b] are 0.  N = n_frames, or the largest total (one small device-to-host copy).  reverse: each utterance's
    rows in reversed time (row n = its frame total_b - 1 - n), the order an odd flow decodes in."""
    B, Lt = _durations_arg(durations)
    il = lengths_arg(in_lens, "in_lens", B, Lt)
    if il is None:
        raise ValueError("in_lens must be given")
    if n_frames is not None and (isinstance(n_frames, bool) or not isinstance(n_frames, numbers.Integral) or n_frames < 1):
        raise ValueError("n_frames must be a positive integer, got %r" % (n_frames,))
    L.require_cuda(durations)
    dev = durations.device
    in32 = torch.tensor(il, dtype=torch.int32, device=dev)
    if n_frames is None:
        live = torch.arange(Lt, device=dev)[None, :] < in32[:, None]
        n_frames = max(int((durations.clamp(min=0) * live).sum(1).max().item()), 1)
    return ops.durations_to_rows(durations.to(torch.int32).contiguous(), in32, int(n_frames), reverse)


def scale_durations(durations, in_lens, pace, min_frames=1):
    """Durations at another speaking rate.  pace: a positive number, or one per utterance; above 1 is faster (frames ~ frames /
    pace).  With e_l the running end of token l:  e'_l = floor(e_l / pace + 0.5) in float64, then for ascending l
    e'_l = max(e'_l, e'_{l-1} + min_frames), and d'_l = e'_l - e'_{l-1}: rounding the ENDS keeps the whole utterance at
    round(T / pace) frames, wherever min_frames does not force more.  pace 1 is the identity when every d_l >= min_frames.
    durations [B, L] integers (device or host; negatives count as 0; read to the host once)
    -> (durations' [B, L] int32 on the device of `durations`, zeros behind in_lens[b]; totals: CPU int64 [B])."""
    B, Lt = _durations_arg(durations)
    il = lengths_arg(in_lens, "in_lens", B, Lt)
    if il is None:
        raise ValueError("in_lens must be given")
    if isinstance(min_frames, bool) or not isinstance(min_frames, numbers.Integral) or min_frames < 0:
        raise ValueError("min_frames must be a non-negative integer, got %r" % (min_frames,))
    if torch.is_tensor(pace):
        pace = pace.reshape(-1).tolist()
    if isinstance(pace, (list, tuple)):
        if len(pace) != B:
            raise ValueError("pace has %d entries for a batch of %d" % (len(pace), B))
        paces = [float(p) for p in pace]
    elif isinstance(pace, numbers.Real) and not isinstance(pace, bool):
        paces = [float(pace)] * B
    else:
        raise ValueError("pace must be a positive number or one per utterance, got %r" % (pace,))
    if any(not (p > 0.0 and math.isfinite(p)) for p in paces):
        raise ValueError("pace must be positive and finite, got %r" % (pace,))
    host = durations.detach().cpu().tolist()
    out = torch.zeros(B, Lt, dtype=torch.int32)
    totals = []
    for b in range(B):
        end = new_end = 0
        for l in range(il[b]):
            end += max(int(host[b][l]), 0)
            e = max(int(math.floor(end / paces[b] + 0.5)), new_end + int(min_frames))
            out[b, l] = e - new_end
            new_end = e
        totals.append(new_end)
    return out.to(durations.device), torch.tensor(totals, dtype=torch.int64)
