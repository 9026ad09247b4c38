"""F0 tracking on the device (YIN; additive: the reference has no pitch tracker; csrc/pitch.hip).

    audio = stft.mel_to_audio_ragged(mel, lengths)                              # [B, hop (T - 1)], zeros behind an utterance
    f0, aperiodicity = pitch.f0(audio, [hop * (n - 1) for n in lengths], hop_length=hop)   # [B, T] Hz, 0 = unvoiced; one launch
    n_voiced, mean, std = pitch.f0_statistics(f0)                               # per utterance, semitones re 1 Hz

Frame t is centred on sample t * hop_length, so Griffin-Lim's hop * (T - 1) samples give T frames, one per mel frame, and
metrics.f0_distortion compares two contours along the path of metrics.mel_cepstral_distortion(..., return_path=True).
Everything runs on the device and refuses tensors on the host."""
from __future__ import annotations

import math
import numbers

import torch

from . import _lib as L
from . import ops
from .metrics import MAX_LAG
from .model import lengths_arg

MAX_WINDOW = 2048          # ft_f0_yin_ragged: the integration window (even), and metrics.MAX_LAG = 1022 for the longest lag


def _int_arg(v, name, lo=1):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < lo:
        raise ValueError("%s must be an integer >= %d, got %r" % (name, lo, v))
    return int(v)


def _real_arg(v, name):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v <= 0:
        raise ValueError("%s must be a positive number, got %r" % (name, v))
    return float(v)


def lag_range(sampling_rate, fmin, fmax):
    """-> (tau_min, tau_max) = (floor(sr / fmax), ceil(sr / fmin)), the lags f0() searches"""
    return int(math.floor(sampling_rate / fmax)), int(math.ceil(sampling_rate / fmin))


def f0(audio, n_samples=None, sampling_rate=22050, hop_length=256, win_length=1024, fmin=60.0, fmax=400.0, threshold=0.15):
    """Fundamental frequency by YIN (de Cheveigne & Kawahara 2002: difference function, cumulative mean normalisation,
    absolute threshold, parabolic interpolation), the whole zero-padded batch in one launch: audio [N] or [B, N] (fp32 on the
    device, any strides), n_samples its samples per utterance, 1 ..= N (None: N) -> (f0 in Hz with 0 = unvoiced,
    aperiodicity = d' at the chosen lag, or its least value over the lag range where unvoiced), both [B, T] fp32 ([T] for
    [N]), T = N // hop_length + 1.  Utterance b has n_samples[b] // hop_length + 1 frames, frame t is centred on sample
    t * hop_length (it integrates win_length samples from t * hop_length - win_length / 2 on, against their copies up to
    tau_max + 1 = ceil(sr / fmin) + 1 samples later); samples outside the utterance count as 0 and are never read, frames
    behind an utterance's are 0.  Lags tau_min = floor(sr / fmax) ..= tau_max.  All arithmetic is fp32, one rounding per
    operation, so a float32 replay gives the same bits (include/flowtron_hip.h states the rule).  A frame whose window holds
    NaN or inf gives f0 = 0.  NotImplementedError for win_length > 2048 or odd, or tau_max > 1022 (metrics.MAX_LAG)."""
    if not torch.is_tensor(audio) or audio.dim() not in (1, 2):
        raise ValueError("audio must be a [N] or [B, N] tensor, got %s" % ((tuple(audio.shape) if torch.is_tensor(audio) else type(audio).__name__),))
    if min(audio.shape) < 1:
        raise ValueError("audio must hold at least one utterance and one sample, got shape %s" % (tuple(audio.shape),))
    if audio.dtype != torch.float32:
        raise ValueError("audio must be float32, got %s" % audio.dtype)
    single = audio.dim() == 1
    a2 = audio[None] if single else audio
    B, N = a2.shape
    sr = _real_arg(sampling_rate, "sampling_rate")
    hop = _int_arg(hop_length, "hop_length")
    W = _int_arg(win_length, "win_length")
    lo, hi = _real_arg(fmin, "fmin"), _real_arg(fmax, "fmax")
    if not lo <= hi:
        raise ValueError("fmin must not exceed fmax, got %r and %r" % (fmin, fmax))
    if isinstance(threshold, bool) or not isinstance(threshold, numbers.Real) or not 0 < threshold <= 1:
        raise ValueError("threshold must lie in (0, 1], got %r" % (threshold,))
    tau_min, tau_max = lag_range(sr, lo, hi)
    if tau_min < 2:
        raise ValueError("fmax = %r is above half the sampling rate %r: the shortest lag must be at least 2 samples" % (fmax, sampling_rate))
    ln = lengths_arg(n_samples, "n_samples", B, N)
    if W > MAX_WINDOW or W % 2 or tau_max > MAX_LAG:
        raise NotImplementedError("f0 holds an even win_length of at most %d samples (MAX_WINDOW) and lags up to %d (metrics.MAX_LAG), "
                                  "got win_length %d and ceil(sampling_rate / fmin) = %d" % (MAX_WINDOW, MAX_LAG, W, tau_max))
    if B > 65535:
        raise NotImplementedError("f0 holds at most 65535 utterances a call, got %d" % B)
    L.require_cuda(a2)
    n32 = torch.tensor(ln if ln is not None else [N] * B, dtype=torch.int32, device=a2.device)
    out, ap = ops.f0_yin_ragged(a2.detach(), n32, sr, hop, W, tau_min, tau_max, float(threshold))
    return (out[0], ap[0]) if single else (out, ap)


def f0_statistics(f0, lens=None):
    """The pitch of each utterance in one line: f0 [B, T] (or [T]) in Hz with 0 = unvoiced, lens its frames (None: T) ->
    (n_voiced [B] int64, mean [B] float64, std [B] float64): count, mean and (population) standard deviation of
    12 log2(f0) -- semitones re 1 Hz -- over the voiced frames, NaN where nothing is voiced.  The spread is the number that
    goes with a sweep over sigma.  Plain torch on the tensor's device."""
    if not torch.is_tensor(f0) or f0.dim() not in (1, 2) or not f0.dtype.is_floating_point:
        raise ValueError("f0 must be a floating [T] or [B, T] tensor, got %s" % ((tuple(f0.shape) if torch.is_tensor(f0) else type(f0).__name__),))
    f = f0[None] if f0.dim() == 1 else f0
    B, T = f.shape
    if T < 1 or B < 1:
        raise ValueError("f0 must hold at least one utterance and one frame, got shape %s" % (tuple(f0.shape),))
    ln = lengths_arg(lens, "lens", B, T)
    voiced = f > 0
    if ln is not None:
        voiced = voiced & (torch.arange(T, device=f.device)[None, :] < torch.tensor(ln, device=f.device)[:, None])
    st = 12.0 * torch.log2(torch.where(voiced, f.double(), torch.ones((), dtype=torch.float64, device=f.device)))
    n = voiced.sum(1)
    nd = n.double()
    mean = st.sum(1) / nd                                                    # 0 / 0 = NaN where nothing is voiced
    dev = torch.where(voiced, st - mean[:, None], torch.zeros((), dtype=torch.float64, device=f.device))
    std = torch.sqrt((dev * dev).sum(1) / nd)
    return n, mean, std
