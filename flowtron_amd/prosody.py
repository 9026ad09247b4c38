"""Pitch and pace of audio on the device: time-domain pitch-synchronous overlap-add (TD-PSOLA) on the F0 track (additive: the
reference has no F0 input and no way to change the pitch; csrc/prosody.hip).

    audio = stft.mel_to_audio_ragged(mel, lengths)                               # or a recording
    audio, n = level.trim(audio, n_samples)
    f0, _ = pitch.f0_track(audio, n, hop_length=hop)                             # [B, T] Hz, 0 = unvoiced
    ratio = prosody.pitch_ratio(f0, shift_semitones=3.0, range_scale=0.5)        # [B, T]: three semitones up, half the range
    out, n_out = prosody.modify(audio, n, f0, hop_length=hop, pitch_ratio=ratio, pace=1.1)
    mel = stft.mel_spectrogram_ragged(out, n_out)                                # n_out is an int32 tensor on the device

Two-period Hann grains are cut at analysis marks one F0 period apart (integrated from the track: no search for glottal pulses)
and laid down again at synthesis marks period / ratio apart, each taking the grain whose analysis mark is nearest in the
input's time: the fundamental moves, the spectral envelope stays, and pace moves along the input faster or slower without
re-synthesis.  Positions are integers in 1/256 sample, the window a host-made table, every fp32 operation rounded on its own:
include/flowtron_hip.h states the rule and tests/prosody_ref.py replays it bit for bit.  Every utterance gives the same bits
alone as in any batch; nothing here synchronises with the host.  What the tests pin is F0, envelope, length and bits, not how
it sounds; no outside PSOLA implementation was available to compare with."""
from __future__ import annotations

import collections
import math
import numbers

import numpy as np
import torch

from . import _lib as L
from .level import _audio_arg, _lengths

Q = 256                    # FT_PSOLA_Q: positions are integers in 1 / Q sample
MIN_RATIO, MAX_RATIO = 0.625, 2.0          # below 0.625 neighbouring two-period grains stop overlapping (0.19 between marks there)
MIN_PACE, MAX_PACE = 0.25, 4.0
MIN_PERIOD, MAX_PERIOD = 16, 1024          # FT_PSOLA_MIN_PERIOD / FT_PSOLA_MAX_PERIOD, samples
MAX_SAMPLES = 1 << 22      # FT_PSOLA_MAX_SAMPLES: N and N_out (positions stay below 2^31)
MAX_BATCH = 65535
HANN_STEPS = 1024          # FT_PSOLA_HANN: the window table holds HANN_STEPS + 1 values

Marks = collections.namedtuple("Marks", "analysis n_analysis synthesis source half n_synthesis n_out")


# ---- host pieces (tests/prosody_ref.py uses these very functions) ---------------------------------------------------------------

def hann_table():
    """-> [1025] float64: 0.5 + 0.5 cos(pi i / 1024), the falling half of the window; the kernels take it rounded once to fp32"""
    return 0.5 + 0.5 * np.cos(np.pi * np.arange(HANN_STEPS + 1, dtype=np.float64) / HANN_STEPS)


def pace_q(pace):
    """the pace in 1 / 65536: the nearest integer, halves to even"""
    return int(round(float(pace) * 65536.0))


def default_unvoiced_period(sampling_rate):
    """the grain spacing where nothing is voiced: 5 ms"""
    return int(round(float(sampling_rate) / 200.0))


def out_samples(n, pace):
    """the samples of an utterance of n at this pace: max(1, (n << 16) // pace_q(pace))"""
    return max(1, (int(n) << 16) // pace_q(pace))


# ---- argument checks ----------------------------------------------------------------------------------------------------------------

def _args(who, audio, n_samples, f0, sampling_rate, hop_length, pitch_ratio, pace, unvoiced_period):
    a2, single = _audio_arg(audio, who)
    B, N = a2.shape
    if isinstance(sampling_rate, bool) or not isinstance(sampling_rate, numbers.Real) or not math.isfinite(sampling_rate) or sampling_rate <= 0:
        raise ValueError("sampling_rate must be a positive number, got %r" % (sampling_rate,))
    sr256 = float(np.float32(float(sampling_rate) * 256.0))
    if isinstance(hop_length, bool) or not isinstance(hop_length, numbers.Integral) or hop_length < 1:
        raise ValueError("hop_length must be an integer >= 1, got %r" % (hop_length,))
    hop = int(hop_length)
    if not torch.is_tensor(f0) or f0.dtype != torch.float32 or f0.dim() != a2.dim() - (1 if single else 0) or \
            (f0[None] if single else f0).shape[0] != B:
        raise ValueError("f0 must be a float32 %s tensor as pitch.f0_track returns it, got %s"
                         % ("[T]" if single else "[%d, T]" % B, (tuple(f0.shape), f0.dtype) if torch.is_tensor(f0) else type(f0).__name__))
    f2 = (f0[None] if single else f0).detach()
    T = f2.shape[1]
    if T < N // hop + 1:
        raise ValueError("f0 must hold at least N // hop_length + 1 = %d frames (frame t is centred on sample t * hop_length), got %d"
                         % (N // hop + 1, T))
    if unvoiced_period is None:
        unv = default_unvoiced_period(sampling_rate)
    elif isinstance(unvoiced_period, bool) or not isinstance(unvoiced_period, numbers.Integral):
        raise ValueError("unvoiced_period must be an integer number of samples or None, got %r" % (unvoiced_period,))
    else:
        unv = int(unvoiced_period)
    if not MIN_PERIOD <= unv <= MAX_PERIOD:
        raise NotImplementedError("%s holds an unvoiced_period of %d .. %d samples, got %d" % (who, MIN_PERIOD, MAX_PERIOD, unv))
    if isinstance(pace, numbers.Real) and not isinstance(pace, bool):
        paces = [float(pace)] * B
    else:
        try:
            paces = [float(p) for p in pace]
        except TypeError:
            raise ValueError("pace must be a number or a sequence of %d numbers, got %r" % (B, pace))
        if len(paces) != B:
            raise ValueError("pace must be a number or a sequence of %d numbers, got %d" % (B, len(paces)))
    for p in paces:
        if not MIN_PACE <= p <= MAX_PACE:                                   # (NaN fails both)
            raise ValueError("pace must lie in [%g, %g], got %r" % (MIN_PACE, MAX_PACE, p))
    N_out = out_samples(N, min(paces))
    if N > MAX_SAMPLES or N_out > MAX_SAMPLES:
        raise NotImplementedError("%s holds at most %d samples an utterance (MAX_SAMPLES = 2^22) before and after, got N = %d and N_out = %d"
                                  % (who, MAX_SAMPLES, N, N_out))
    if torch.is_tensor(pitch_ratio):
        r = pitch_ratio.detach()
        if r.dtype != torch.float32 or r.dim() > 2 or (r.dim() == 2 and single and r.shape[0] != 1):
            raise ValueError("pitch_ratio must be a number or a float32 [B] or [B, T] tensor, got %s %s" % (tuple(r.shape), r.dtype))
        if single and r.dim() == 1 and r.shape[0] == T:
            r = r[None]                                                     # the [T] of an [N]
        if r.dim() == 0:
            r = r.reshape(1, 1).expand(B, T)
        elif r.dim() == 1:
            if r.shape[0] != B:
                raise ValueError("pitch_ratio [B] must hold %d entries, got %d" % (B, r.shape[0]))
            r = r[:, None].expand(B, T)
        elif tuple(r.shape) != (B, T):
            raise ValueError("pitch_ratio [B, T] must have f0's shape %s, got %s" % ((B, T), tuple(r.shape)))
    elif isinstance(pitch_ratio, numbers.Real) and not isinstance(pitch_ratio, bool) and math.isfinite(pitch_ratio):
        r = float(pitch_ratio)
    else:
        raise ValueError("pitch_ratio must be a finite number or a float32 [B] or [B, T] tensor, got %r" % (pitch_ratio,))
    return a2, single, f2, r, paces, N_out, sr256, hop, unv


_HANN = {}                 # device -> the window table on it: made once, so a warm call copies one small vector of paces only


def _hann(device):
    key = str(device)
    if key not in _HANN:
        _HANN[key] = torch.from_numpy(hann_table().astype(np.float32)).to(device)
    return _HANN[key]


def _marks(a2, n32, f2, r, paces, N_out, sr256, hop, unv):
    B, N = a2.shape
    T = f2.shape[1]
    dev = a2.device
    L.require_cuda(f2)
    if not torch.is_tensor(r):
        r = torch.full((1, 1), r, dtype=torch.float32, device=dev).expand(B, T)
    L.require_cuda(r)
    KA, KS = -(-N // MIN_PERIOD), -(-N_out // (MIN_PERIOD // 2))
    if min(paces) == max(paces):                                            # one pace: a fill, nothing is copied from the host
        pq = torch.full((B,), pace_q(paces[0]), dtype=torch.int32, device=dev)
    else:
        pq = torch.tensor([pace_q(p) for p in paces], dtype=torch.int32, device=dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    m = Marks(i32(B, KA), i32(B), i32(B, KS), i32(B, KS), i32(B, KS), i32(B), i32(B))
    L.check(L.lib().ft_psola_marks(L.ptr(f2), *f2.stride(), L.ptr(r), *r.stride(), L.ptr(n32), L.ptr(pq), L.ptr(m.analysis),
                                   L.ptr(m.n_analysis), L.ptr(m.synthesis), L.ptr(m.source), L.ptr(m.half), L.ptr(m.n_synthesis),
                                   L.ptr(m.n_out), B, N, N_out, T, hop, KA, KS, sr256, unv, L.stream()), "ft_psola_marks")
    return m


# ---- the public calls ---------------------------------------------------------------------------------------------------------------

def marks(audio, n_samples, f0, sampling_rate=22050, hop_length=256, pitch_ratio=1.0, pace=1.0, unvoiced_period=None):
    """Where modify() cuts and where it lays down, the same arguments -> Marks(analysis [B, ceil(N / 16)], n_analysis [B],
    synthesis, source, half [B, ceil(N_out / 8)], n_synthesis [B], n_out [B]), int32 on the device (no leading B for [N]):
    positions in 1/256 sample; grain j is centred on (synthesis[j] + 128) >> 8 of the output, reads around
    (analysis[source[j]] + 128) >> 8 of the input and is half[j] samples wide to either side.  Entries behind an utterance's
    counts are not written.  One entry call (one launch: a wave per utterance)."""
    a2, single, f2, r, paces, N_out, sr256, hop, unv = _args("marks", audio, n_samples, f0, sampling_rate, hop_length, pitch_ratio,
                                                             pace, unvoiced_period)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    m = _marks(a2, n32, f2, r, paces, N_out, sr256, hop, unv)
    return Marks(*[x[0] for x in m]) if single else m


def modify(audio, n_samples, f0, sampling_rate=22050, hop_length=256, pitch_ratio=1.0, pace=1.0, unvoiced_period=None):
    """Change the pitch and the pace of a zero-padded batch: audio [N] or [B, N] fp32 on the device (any strides), n_samples a
    host sequence or an int32 tensor on the device (clamped to 1 ..= N; nothing behind an utterance's end is read), f0
    [B, T] Hz with 0 = unvoiced as pitch.f0 / pitch.f0_track return it at this hop_length (frame t centred on sample
    t * hop_length, T >= N // hop_length + 1, further frames ignored; NaN, inf and values <= 0 count as unvoiced)
    -> (out [B, N_out] fp32 with zeros behind each utterance, n_out int32 [B] on the device = max(1, (n << 16) // pace_q)).
    pitch_ratio: the factor on F0, a number, a [B] or a [B, T] fp32 tensor on the device (pitch_ratio() makes one), clamped to
    [0.625, 2]; unvoiced frames are never shifted, their grains are unvoiced_period samples apart (None: 5 ms).  pace: a
    number or B numbers in [0.25, 4], above 1 is faster (as align.scale_durations); N_out is out_samples(N, the smallest
    pace).  With pitch_ratio = 1 and pace = 1 the output is the input to within 1e-6 for |x| <= 1.  Two entry calls
    (ft_psola_marks, ft_psola_synth: a launch each), nothing on the host between them.
    NotImplementedError for N or N_out above 2^22 samples, more than 65,535 utterances, an unvoiced_period outside 16 .. 1024."""
    a2, single, f2, r, paces, N_out, sr256, hop, unv = _args("modify", audio, n_samples, f0, sampling_rate, hop_length, pitch_ratio,
                                                             pace, unvoiced_period)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    m = _marks(a2, n32, f2, r, paces, N_out, sr256, hop, unv)
    B, N = a2.shape
    out = torch.empty(B, N_out, dtype=torch.float32, device=a2.device)
    L.check(L.lib().ft_psola_synth(L.ptr(a2), *a2.stride(), L.ptr(n32), L.ptr(m.analysis), L.ptr(m.synthesis), L.ptr(m.source),
                                   L.ptr(m.half), L.ptr(m.n_synthesis), L.ptr(m.n_out), L.ptr(_hann(a2.device)), L.ptr(out), B, N,
                                   N_out, m.analysis.shape[1], m.synthesis.shape[1], L.stream()), "ft_psola_synth")
    return (out[0], m.n_out[0]) if single else (out, m.n_out)


def pitch_ratio(f0, lens=None, shift_semitones=0.0, range_scale=1.0):
    """The per-frame factor that moves and scales an utterance's intonation: f0 [B, T] (or [T]) Hz with 0 = unvoiced, lens its
    frames (None: T) -> [B, T] fp32.  On a voiced frame the target is log f0' = mean + range_scale (log f0 - mean) + shift,
    mean the utterance's voiced-frame mean of log f0 (the one pitch.f0_statistics reports), and the result f0' / f0; 1 on an
    unvoiced frame.  range_scale = 0 is a monotone reading, 2 twice the range.  Plain float64 torch on the tensor's device,
    rounded once; no synchronisation."""
    if not torch.is_tensor(f0) or f0.dim() not in (1, 2) or not f0.dtype.is_floating_point or min(f0.shape) < 1:
        raise ValueError("f0 must be a floating [T] or [B, T] tensor, got %s" % ((tuple(f0.shape) if torch.is_tensor(f0) else type(f0).__name__),))
    for v, name in ((shift_semitones, "shift_semitones"), (range_scale, "range_scale")):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
            raise ValueError("%s must be a finite number, got %r" % (name, v))
    f = f0[None] if f0.dim() == 1 else f0
    B, T = f.shape
    voiced = (f > 0) & torch.isfinite(f)
    if lens is not None:
        if torch.is_tensor(lens):
            ln = lens.to(f.device).reshape(B)
        else:
            if len(lens) != B:
                raise ValueError("lens must hold %d entries, got %d" % (B, len(lens)))
            ln = torch.tensor([int(v) for v in lens], device=f.device)
        voiced = voiced & (torch.arange(T, device=f.device)[None, :] < ln[:, None])
    one = torch.ones((), dtype=torch.float64, device=f.device)
    lf = torch.log2(torch.where(voiced, f.double(), one))
    mean = (lf.sum(1) / voiced.sum(1).double())[:, None]                     # NaN where nothing is voiced: no frame reads it
    target = mean + float(range_scale) * (lf - mean) + float(shift_semitones) / 12.0
    ratio = torch.where(voiced, torch.exp2(target - lf), one).to(torch.float32)
    return ratio[0] if f0.dim() == 1 else ratio
