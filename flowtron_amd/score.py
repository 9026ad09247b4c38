"""Scoring utterances on the device: the exact log-likelihood of every mel frame, and the health of attention maps
(additive: the reference exposes the likelihood only as FlowtronLoss's batch mean, and its attention only as plots).

Corpus cleaning and held-out evaluation -- rank recordings, see where a likelihood collapses, check that the teacher-forced
attention walked the whole text:
    ll = model.log_likelihood(mel, speaker_ids, text, in_lens, out_lens)               # frame_ll [B,T], total [B], nll_per_dim [B]
    z, attn, logp = model.alignments(mel, speaker_ids, text, in_lens, out_lens)        # every flow in natural time
    diag = attention_diagnostics(attn, in_lens, out_lens)
    ok = healthy(diag, in_lens)                                                        # bool [F, B] on the device

Robust synthesis -- draw several z for one sentence, decode them in one batched pass, keep a sample whose attention is healthy:
    mel, aws, lengths = model.infer(residual, speaker_ids, text, return_lengths=True)  # B candidates
    maps = infer_attention_maps(aws, lengths)                                          # [F, B, N', L] in natural time
    ok = healthy(attention_diagnostics(maps, [L] * B, lengths), [L] * B)

Both reductions run in csrc/score.hip (include/flowtron_hip.h states their rules and summation orders; tests/score_ref.py
replays them) and refuse tensors on the host."""
from __future__ import annotations

import collections
import ctypes as C
import math
import numbers

import torch

from . import _lib as L
from . import ops
from .model import lengths_arg

MAX_FLOWS, MAX_MEL = 8, 128            # ft_frame_loglik: log_s pointers per call, channels per frame

LogLikelihood = collections.namedtuple("LogLikelihood", "frame_ll total nll_per_dim")
FrameLogLikelihood = collections.namedtuple("FrameLogLikelihood", "frame_ll total")
AttentionDiagnostics = collections.namedtuple(
    "AttentionDiagnostics", "peaks n_attended n_backward n_skipped longest_run first_peak last_peak focus coverage")


def gaussian_constant(M, sigma):
    """(M / 2) ln(2 pi sigma^2), as ft_frame_loglik forms it on the host"""
    return M * 0.5 * math.log(6.283185307179586 * sigma * sigma)


def _sigma_arg(sigma):
    if isinstance(sigma, bool) or not isinstance(sigma, numbers.Real) or not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError("sigma must be a positive finite number, got %r" % (sigma,))
    return float(sigma)


def frame_log_likelihood(z, log_s_list, out_lens, sigma=1.0, reversed=None):
    """The kernel on given tensors: z [T, B, M] and log_s_list (1 to 8 tensors [T, B, M], last stride 1, all with one row stride:
    the strided views of the coupling outputs are read in place), time-major fp32 on the device -- elements 0 and 1 of the
    forward's tuple.  out_lens: a list or an integer tensor on the host or the device, 1 ..= T.  reversed: one flag per log_s,
    true where it is in its flow's reversed time (None: the odd ones, as Flowtron builds its flows).
    -> (frame_ll [B, T] float64: the log-density of frame t of utterance b in nats, natural time, 0 behind out_lens[b];
    total [B] float64: their sum).  Utterance b comes out with the same bits alone as inside any batch."""
    if not torch.is_tensor(z) or z.dim() != 3:
        raise ValueError("z must be a [T, B, M] tensor, got %s" % (tuple(z.shape) if torch.is_tensor(z) else type(z).__name__,))
    T, B, M = z.shape
    if T < 1 or B < 1 or not 1 <= M <= MAX_MEL:
        raise ValueError("z must hold at least one frame and utterance and 1 ..= %d channels, got shape %s" % (MAX_MEL, tuple(z.shape)))
    log_s_list = list(log_s_list)
    if not 1 <= len(log_s_list) <= MAX_FLOWS:
        raise ValueError("log_s_list must hold 1 ..= %d tensors, got %d" % (MAX_FLOWS, len(log_s_list)))
    for f, ls in enumerate(log_s_list):
        if not torch.is_tensor(ls) or tuple(ls.shape) != (T, B, M):
            raise ValueError("log_s_list[%d] must be a tensor of z's shape %s, got %s"
                             % (f, (T, B, M), tuple(ls.shape) if torch.is_tensor(ls) else type(ls).__name__))
    if z.dtype != torch.float32 or any(ls.dtype != torch.float32 for ls in log_s_list):
        raise ValueError("z and log_s must be float32")
    if reversed is None:
        reversed = [f % 2 == 1 for f in range(len(log_s_list))]
    reversed = list(reversed)
    if len(reversed) != len(log_s_list):
        raise ValueError("reversed has %d flags for %d log_s tensors" % (len(reversed), len(log_s_list)))
    sigma = _sigma_arg(sigma)
    ol = lengths_arg(out_lens, "out_lens", B, T)
    if ol is None:
        raise ValueError("out_lens must be given")
    L.require_cuda(z, *log_s_list)
    z = z.detach()
    z = z if z.is_contiguous() else z.contiguous()
    views = []
    for ls in log_s_list:
        ls = ls.detach()
        # a [T, B, M] view of rows ld apart ([T*B, ld] underneath) is read in place; anything else is copied once
        if ls.stride(2) != 1 or ls.stride(1) < M or ls.stride(0) != ls.stride(1) * B:
            ls = ls.contiguous()
        views.append(ls)
    ld = int(views[0].stride(1))
    if any(int(v.stride(1)) != ld for v in views):
        views = [v.contiguous() for v in views]
        ld = M
    dev = z.device
    out32 = torch.tensor(ol, dtype=torch.int32, device=dev)
    frame_ll = torch.empty(B, T, dtype=torch.float64, device=dev)
    total = torch.empty(B, dtype=torch.float64, device=dev)
    ptrs = (C.c_void_p * len(views))(*[v.data_ptr() for v in views])
    rev = (C.c_int32 * len(views))(*[int(bool(r)) for r in reversed])
    L.check(L.lib().ft_frame_loglik(L.ptr(z), ptrs, rev, len(views), ld, L.ptr(out32), sigma, L.ptr(frame_ll), L.ptr(total),
                                    T, B, M, L.stream()), "ft_frame_loglik")
    return FrameLogLikelihood(frame_ll, total)


def log_likelihood(model, mel, speaker_ids, text, in_lens, out_lens, attn_prior=None, sigma=1.0):
    """Flowtron.log_likelihood (see there)."""
    if hasattr(model, "gaussian_mixture"):
        raise NotImplementedError("log_likelihood scores the standard-normal prior only: this model was built with n_components > 1, "
                                  "whose mixture prior has its own likelihood kernels (csrc/mixture.hip)")
    sigma = _sigma_arg(sigma)
    out, unsort, il, ol = model._forward_any_order("log_likelihood", mel, speaker_ids, text, in_lens, out_lens, attn_prior)
    order = sorted(range(len(il)), key=lambda b: -il[b])                     # the order the forward saw (_forward_any_order)
    reversed_ = [hasattr(flow, "ar_step") for flow in model.flows]          # an AR_Back_Step runs on the flipped utterance
    with torch.no_grad():
        z, log_s = out[0], out[1]
        M = z.shape[2]
        fl = frame_log_likelihood(z, log_s, [ol[b] for b in order], sigma, reversed_)
        frame_ll, total = unsort(fl.frame_ll), unsort(fl.total)
        n = torch.tensor(ol, dtype=torch.float64, device=z.device)
        nll = -(total + n * gaussian_constant(M, sigma)) / (n * M)
    return LogLikelihood(frame_ll, total, nll)


def attention_diagnostics(attn, in_lens, out_lens):
    """attn [F, B, T, L] or [B, T, L] fp32 on the device, any strides, NATURAL time (what Flowtron.alignments and
    infer_attention_maps return); in_lens / out_lens: lists or integer tensors on the host or the device, 1 ..= L and 1 ..= T.
    With peak[t] the token of frame t's largest weight (the lowest on a tie) ->
      peaks [F, B, T] int32 (-1 behind out_lens[b]) and per (flow, utterance), int32 [F, B]:
      n_attended: distinct tokens that are some frame's peak;  n_backward: frames whose peak lies before the previous frame's;
      n_skipped: tokens jumped over, sum of max(peak[t] - peak[t-1] - 1, 0);  longest_run: the most consecutive frames on one peak;
      first_peak, last_peak;  and float64 [F, B]:  focus = the mean of the peak weights,  coverage = n_attended / in_lens[b].
    A [B, T, L] input gives the same fields without the flow dimension."""
    if not torch.is_tensor(attn) or attn.dim() not in (3, 4):
        raise ValueError("attn must be a [F, B, T, L] or [B, T, L] tensor, got %s"
                         % (tuple(attn.shape) if torch.is_tensor(attn) else type(attn).__name__,))
    single = attn.dim() == 3
    a = attn[None] if single else attn
    F_, B, T, Lt = a.shape
    if min(F_, B, T, Lt) < 1:
        raise ValueError("attn must hold at least one flow, utterance, frame and token, got shape %s" % (tuple(attn.shape),))
    if a.dtype != torch.float32:
        raise ValueError("attn must be float32, got %s" % a.dtype)
    il = lengths_arg(in_lens, "in_lens", B, Lt)
    ol = lengths_arg(out_lens, "out_lens", B, T)
    if il is None or ol is None:
        raise ValueError("in_lens and out_lens must be given")
    L.require_cuda(a)
    a = a.detach()
    dev = a.device
    in32 = torch.tensor(il, dtype=torch.int32, device=dev)
    out32 = torch.tensor(ol, dtype=torch.int32, device=dev)
    peaks, counters, focus_sum = ops.attn_diagnostics(a, in32, out32)
    focus = focus_sum / out32.to(torch.float64)[None, :]
    coverage = counters[..., 0].to(torch.float64) / in32.to(torch.float64)[None, :]
    fields = [peaks] + [counters[..., k] for k in range(6)] + [focus, coverage]
    if single:
        fields = [x[0] for x in fields]
    return AttentionDiagnostics(*fields)


def infer_attention_maps(attention_weights, lengths):
    """What Flowtron.infer(..., return_lengths=True) returns -> the maps [F, B, N', L] fp32 in natural time, zeros behind each
    utterance's frames.  attention_weights: per decoded flow a list of N' rows [B, 1, L]; list k belongs to flow F - 1 - k (infer
    walks the flows in reverse), and row i is the i-th DECODED frame: for an odd flow, natural frame lengths[b] - 1 - i.
    lengths: the frames of every utterance (list or integer tensor, 1 ..= N')."""
    if not isinstance(attention_weights, (list, tuple)) or not attention_weights:
        raise ValueError("attention_weights must be infer's list of per-flow row lists")
    F_ = len(attention_weights)
    per_flow = []
    for k, rows in enumerate(attention_weights):
        if not isinstance(rows, (list, tuple)) or not rows or not all(torch.is_tensor(r) for r in rows):
            raise ValueError("attention_weights[%d] must be a non-empty list of rows [B, 1, L]" % k)
        a = torch.stack(list(rows))                                          # [N', B, 1, L]
        if a.dim() != 4 or a.shape[2] != 1:
            raise ValueError("attention_weights[%d] must stack to [N', B, 1, L], got %s" % (k, tuple(a.shape)))
        per_flow.append(a[:, :, 0].permute(1, 0, 2))                         # [B, N', L]
    B, N, Lt = per_flow[0].shape
    if any(tuple(a.shape) != (B, N, Lt) for a in per_flow):
        raise ValueError("every flow must hold the same rows, got %s" % ([tuple(a.shape) for a in per_flow],))
    nf = lengths_arg(lengths, "lengths", B, N)
    if nf is None:
        raise ValueError("lengths must be given")
    L.require_cuda(*per_flow)
    dev = per_flow[0].device
    n32 = torch.tensor(nf, dtype=torch.int32, device=dev)
    pad = (torch.arange(N, device=dev)[None, :] >= n32[:, None])[:, :, None]                 # [B, N', 1]
    maps = [None] * F_
    with torch.no_grad():
        for k, a in enumerate(per_flow):
            f = F_ - 1 - k
            a = a.detach().float().masked_fill(pad, 0.0).contiguous()
            if f % 2 == 1:
                a = ops.reverse_by_length(a, n32, False)
            maps[f] = a
        return torch.stack(maps)


def healthy(diag, in_lens, max_backward=0, max_skipped=0, min_coverage=1.0, require_end=True, max_run=None):
    """diag: attention_diagnostics' result -> bool [F, B] (or [B]) on the device: true where the attention made at most
    max_backward backward steps, jumped over at most max_skipped tokens, peaked on at least min_coverage of the text, ended on the
    last token (require_end: last_peak == in_lens[b] - 1) and stayed at most max_run frames on one token (None: no limit).
    The thresholds are the caller's; the defaults are the strict reading."""
    B = diag.last_peak.shape[-1]
    il = lengths_arg(in_lens, "in_lens", B, 2 ** 31 - 1)
    if il is None:
        raise ValueError("in_lens must be given")
    in32 = torch.tensor(il, dtype=torch.int32, device=diag.last_peak.device)
    ok = (diag.n_backward <= max_backward) & (diag.n_skipped <= max_skipped) & (diag.coverage >= min_coverage)
    if require_end:
        ok = ok & (diag.last_peak == in32 - 1)
    if max_run is not None:
        ok = ok & (diag.longest_run <= max_run)
    return ok
