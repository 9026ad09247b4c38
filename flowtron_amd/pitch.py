"""F0 tracking on the device (YIN and probabilistic YIN; additive: the reference has no pitch tracker; csrc/pitch.hip).

    audio = stft.mel_to_audio_ragged(mel, lengths)                              # [B, hop (T - 1)], zeros behind an utterance
    f0, aperiodicity = pitch.f0(audio, [hop * (n - 1) for n in lengths], hop_length=hop)   # [B, T] Hz, 0 = unvoiced; one launch
    n_voiced, mean, std = pitch.f0_statistics(f0)                               # per utterance, semitones re 1 Hz
    f0, voiced_prob = pitch.f0_track(audio, n_samples, hop_length=hop)          # probabilistic YIN: through noise; two launches
    prob, freq = pitch.f0_candidates(audio, n_samples, hop_length=hop)          # [B, T, n_bins]: what the path is chosen from

Frame t is centred on sample t * hop_length, so Griffin-Lim's hop * (T - 1) samples give T frames, one per mel frame, and
metrics.f0_distortion compares two contours along the path of metrics.mel_cepstral_distortion(..., return_path=True).
Everything runs on the device and refuses tensors on the host."""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from . import _lib as L
from . import ops
from .metrics import MAX_LAG
from .model import lengths_arg

MAX_WINDOW = 2048          # ft_f0_yin_ragged: the integration window (even), and metrics.MAX_LAG = 1022 for the longest lag
MAX_BINS = 512             # ft_f0_viterbi_ragged: two states a pitch bin, a lane a state
MAX_BAND = 63              # ft_f0_viterbi_ragged: 2 band + 1 offsets and the voicing in one byte


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


def _audio_args(audio, sampling_rate, hop_length, win_length, fmin, fmax):
    """the checks every tracker starts with -> (audio as [B, N], was it [N], sr, hop, W, fmin, fmax)"""
    if not torch.is_tensor(audio) or audio.dim() not in (1, 2):
        raise ValueError("audio must be a [N] or [B, N] tensor, got %s" % ((tuple(audio.shape) if torch.is_tensor(audio) else type(audio).__name__),))
    if min(audio.shape) < 1:
        raise ValueError("audio must hold at least one utterance and one sample, got shape %s" % (tuple(audio.shape),))
    if audio.dtype != torch.float32:
        raise ValueError("audio must be float32, got %s" % audio.dtype)
    single = audio.dim() == 1
    sr = _real_arg(sampling_rate, "sampling_rate")
    hop = _int_arg(hop_length, "hop_length")
    W = _int_arg(win_length, "win_length")
    lo, hi = _real_arg(fmin, "fmin"), _real_arg(fmax, "fmax")
    if not lo <= hi:
        raise ValueError("fmin must not exceed fmax, got %r and %r" % (fmin, fmax))
    return (audio[None] if single else audio), single, sr, hop, W, lo, hi


def _lag_args(who, a2, n_samples, sr, W, lo, hi, sampling_rate, fmax):
    """the lags, the lengths and the limits of the difference function -> (tau_min, tau_max, lengths or None)"""
    B, N = a2.shape
    tau_min, tau_max = lag_range(sr, lo, hi)
    if tau_min < 2:
        raise ValueError("fmax = %r is above half the sampling rate %r: the shortest lag must be at least 2 samples" % (fmax, sampling_rate))
    ln = lengths_arg(n_samples, "n_samples", B, N)
    if W > MAX_WINDOW or W % 2 or tau_max > MAX_LAG:
        raise NotImplementedError("%s holds an even win_length of at most %d samples (MAX_WINDOW) and lags up to %d (metrics.MAX_LAG), "
                                  "got win_length %d and ceil(sampling_rate / fmin) = %d" % (who, MAX_WINDOW, MAX_LAG, W, tau_max))
    if B > 65535:
        raise NotImplementedError("%s holds at most 65535 utterances a call, got %d" % (who, B))
    return tau_min, tau_max, ln


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
    a2, single, sr, hop, W, lo, hi = _audio_args(audio, sampling_rate, hop_length, win_length, fmin, fmax)
    if isinstance(threshold, bool) or not isinstance(threshold, numbers.Real) or not 0 < threshold <= 1:
        raise ValueError("threshold must lie in (0, 1], got %r" % (threshold,))
    tau_min, tau_max, ln = _lag_args("f0", a2, n_samples, sr, W, lo, hi, sampling_rate, fmax)
    B, N = a2.shape
    L.require_cuda(a2)
    n32 = torch.tensor(ln if ln is not None else [N] * B, dtype=torch.int32, device=a2.device)
    out, ap = ops.f0_yin_ragged(a2.detach(), n32, sr, hop, W, tau_min, tau_max, float(threshold))
    return (out[0], ap[0]) if single else (out, ap)


def beta_cdf(x, a, b):
    """The regularised incomplete beta function I_x(a, b) in float64, by its continued fraction (modified Lentz)."""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    if x > (a + 1.0) / (a + b + 2.0):
        return 1.0 - beta_cdf(1.0 - x, b, a)
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x)) / a
    tiny = 1e-300
    c, d = 1.0, 1.0 - (a + b) * x / (a + 1.0)
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 500):
        for num in (m * (b - m) * x / ((a + 2 * m - 1.0) * (a + 2 * m)), -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1.0))):
            d = 1.0 + num * d
            c = 1.0 + num / c
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = c if abs(c) > tiny else tiny
            h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return front * h


def n_pitch_bins(fmin, fmax, bins_per_semitone):
    return int(math.floor(12 * bins_per_semitone * math.log2(fmax / fmin))) + 1


def transition_band(max_octaves_per_second, bins_per_semitone, hop_length, sampling_rate):
    """how many bins the pitch may move from one frame to the next"""
    return int(math.floor(max_octaves_per_second * 12 * bins_per_semitone * hop_length / sampling_rate + 0.5))


def candidate_tables(sampling_rate, fmin, fmax, bins_per_semitone, beta):
    """-> (cum [101], lag_edges [n_bins + 1], centres [n_bins]) float32 numpy, formed in float64 and rounded once
    (include/flowtron_hip.h, F0 through noise)"""
    n_bins, step = n_pitch_bins(fmin, fmax, bins_per_semitone), 12.0 * bins_per_semitone
    cum = np.array([beta_cdf(i / 100.0, beta[0], beta[1]) for i in range(101)], np.float64)
    edges = np.array([sampling_rate / (fmin * 2.0 ** ((i - 0.5) / step)) for i in range(n_bins + 1)], np.float64)
    centres = np.array([fmin * 2.0 ** (k / step) for k in range(n_bins)], np.float64)
    return cum.astype(np.float32), edges.astype(np.float32), centres.astype(np.float32)


def transition_table(band):
    """-> [2 band + 1] float32 numpy: the triangle (band + 1 - |o - band|) / (band + 1)^2, which sums to 1"""
    o = np.arange(2 * band + 1, dtype=np.float64)
    return ((band + 1 - np.abs(o - band)) / float((band + 1) ** 2)).astype(np.float32)


_TABLES = {}               # (device, settings) -> the tables on the device: made once, so a warm call copies nothing from the host


def _on_device(device, key, make):
    k = (str(device),) + key
    if k not in _TABLES:
        if len(_TABLES) >= 64:
            _TABLES.clear()
        _TABLES[k] = tuple(torch.from_numpy(t).to(device) for t in make())
    return _TABLES[k]


def _candidate_args(who, audio, n_samples, sampling_rate, hop_length, win_length, fmin, fmax, bins_per_semitone, beta, absolute_min_prob):
    a2, single, sr, hop, W, lo, hi = _audio_args(audio, sampling_rate, hop_length, win_length, fmin, fmax)
    bps = _int_arg(bins_per_semitone, "bins_per_semitone")
    if (not isinstance(beta, (tuple, list)) or len(beta) != 2
            or any(isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v <= 0 for v in beta)):
        raise ValueError("beta must be two positive numbers (a, b), got %r" % (beta,))
    if isinstance(absolute_min_prob, bool) or not isinstance(absolute_min_prob, numbers.Real) or not 0 <= absolute_min_prob <= 1:
        raise ValueError("absolute_min_prob must lie in [0, 1], got %r" % (absolute_min_prob,))
    tau_min, tau_max, ln = _lag_args(who, a2, n_samples, sr, W, lo, hi, sampling_rate, fmax)
    n_bins = n_pitch_bins(lo, hi, bps)
    if n_bins > MAX_BINS:
        raise NotImplementedError("%s holds at most %d pitch bins (MAX_BINS: the path search gives every state a lane), got %d from "
                                  "bins_per_semitone = %d over %r .. %r Hz" % (who, MAX_BINS, n_bins, bps, fmin, fmax))
    return a2, single, sr, hop, W, lo, hi, bps, (float(beta[0]), float(beta[1])), float(absolute_min_prob), tau_min, tau_max, ln


def _candidates(a2, ln, sr, hop, W, lo, hi, bps, beta, amp, tau_min, tau_max):
    B, N = a2.shape
    L.require_cuda(a2)
    cum, edges, centres = _on_device(a2.device, ("candidates", sr, lo, hi, bps, beta), lambda: candidate_tables(sr, lo, hi, bps, beta))
    n32 = torch.tensor(ln if ln is not None else [N] * B, dtype=torch.int32, device=a2.device)
    return ops.f0_candidates_ragged(a2.detach(), n32, cum, edges, sr, hop, W, tau_min, tau_max, amp) + (n32, centres)


def f0_candidates(audio, n_samples=None, sampling_rate=22050, hop_length=256, win_length=1024, fmin=60.0, fmax=400.0,
                  bins_per_semitone=10, beta=(2.0, 18.0), absolute_min_prob=0.01):
    """The candidate distribution of probabilistic YIN (Mauch & Dixon 2014), one launch for the zero-padded batch: audio,
    n_samples and the frames as for f0() -> (prob, freq), both [B, T, n_bins] fp32 ([T, n_bins] for [N]).  In place of one
    threshold, the thresholds 0.01 .. 1.00 carry a Beta(beta) prior; each gives its weight to the first trough of d' below it,
    and the global minimum of d' takes absolute_min_prob times the weight of the thresholds no trough is below.  prob[t, k]
    is the mass of the candidates that fell into pitch bin k (its sum over k is the frame's probability of being voiced, <= 1),
    freq[t, k] the parabolically refined frequency of the heaviest of them in Hz, 0 for an empty bin.
    n_bins = floor(12 bins_per_semitone log2(fmax / fmin)) + 1, bin k is centred on fmin 2^(k / (12 bins_per_semitone)).
    Frames behind an utterance's, frames that see NaN or inf, and digital silence are all 0.  fp32 with one rounding per
    operation and host-made tables: a float32 replay gives the same bits (include/flowtron_hip.h states the rule).
    NotImplementedError for win_length > 2048 or odd, lags above 1022 (metrics.MAX_LAG) or more than 512 bins (MAX_BINS)."""
    a2, single, sr, hop, W, lo, hi, bps, bt, amp, tau_min, tau_max, ln = _candidate_args(
        "f0_candidates", audio, n_samples, sampling_rate, hop_length, win_length, fmin, fmax, bins_per_semitone, beta, absolute_min_prob)
    prob, freq = _candidates(a2, ln, sr, hop, W, lo, hi, bps, bt, amp, tau_min, tau_max)[:2]
    return (prob[0], freq[0]) if single else (prob, freq)


def f0_track(audio, n_samples=None, sampling_rate=22050, hop_length=256, win_length=1024, fmin=60.0, fmax=400.0,
             bins_per_semitone=10, beta=(2.0, 18.0), absolute_min_prob=0.01, max_octaves_per_second=35.92, switch_prob=0.01):
    """F0 through noise: f0_candidates(), then the most probable path through a pitch HMM with a voiced and an unvoiced state
    per bin, two launches with nothing on the host between them -> (f0 in Hz with 0 = unvoiced, voiced_prob = the frame's
    candidate mass), both [B, T] fp32 ([T] for [N]); f0 goes into metrics.f0_distortion and f0_statistics as f0()'s does.
    The path moves by at most round(max_octaves_per_second * 12 bins_per_semitone * hop_length / sampling_rate) bins a frame,
    with a triangular weight, and changes its voicing with switch_prob (in [1e-6, 1 - 1e-6]).  A voiced frame returns the
    refined frequency of the heaviest candidate in the path's bin, the bin's centre where the bin held none.  An utterance's
    result does not depend on its batch.  NotImplementedError as for f0_candidates, and for a band of more than 63 bins
    (MAX_BAND: a backpointer is one byte)."""
    a2, single, sr, hop, W, lo, hi, bps, bt, amp, tau_min, tau_max, ln = _candidate_args(
        "f0_track", audio, n_samples, sampling_rate, hop_length, win_length, fmin, fmax, bins_per_semitone, beta, absolute_min_prob)
    mo = _real_arg(max_octaves_per_second, "max_octaves_per_second")
    if isinstance(switch_prob, bool) or not isinstance(switch_prob, numbers.Real) or not 1e-6 <= switch_prob <= 1 - 1e-6:
        raise ValueError("switch_prob must lie in [1e-6, 1 - 1e-6], got %r" % (switch_prob,))
    band = transition_band(mo, bps, hop, sr)
    if band > MAX_BAND:
        raise NotImplementedError("f0_track holds a transition band of at most %d bins (MAX_BAND), got %d from max_octaves_per_second = %r"
                                  % (MAX_BAND, band, max_octaves_per_second))
    prob, freq, voiced, n32, centres = _candidates(a2, ln, sr, hop, W, lo, hi, bps, bt, amp, tau_min, tau_max)
    tri, = _on_device(a2.device, ("transition", band), lambda: (transition_table(band),))
    out = ops.f0_viterbi_ragged(prob, freq, voiced, n32, tri, centres, a2.shape[1], hop, float(switch_prob))
    return (out[0], voiced[0]) if single else (out, voiced)


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
