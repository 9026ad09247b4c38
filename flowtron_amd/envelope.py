"""F0-adaptive spectral envelope (CheapTrick) and its mel-cepstrum on the device: the features the papers' mel-cepstral
distortion is computed on (additive: the reference has no metric of its own; csrc/envelope.hip).

    f0 = pitch.f0_track(audio, n_samples)[0]                                    # [B, T] Hz on the frame grid t * hop
    env = envelope.spectral_envelope(audio, n_samples, f0)                      # [B, T, H + 1] POWER envelope, H = fft_size / 2
    mc = envelope.mel_cepstra(audio, n_samples, f0, order=24)                   # [B, T, 25] c0 .. c24 (SPTK's alpha for the rate)
    mcd = metrics.envelope_cepstral_distortion(a, n_a, f0_a, b, n_b, f0_b)      # dB over c1 .. c24 along the DTW path

A log-mel frame of a 1024-sample Hann window resolves the harmonics, so its cepstra move with F0; the window here is three
periods long, the spectrum is smoothed over 2 F0 / 3 and liftered at the period, and what is left is the vocal tract's part.
audio is [N] or [B, N] fp32 on the device, a zero-padded batch, any strides; n_samples a host sequence of B integers in
1 ..= N or an int32 tensor on the device (clamped in the kernel): nothing here synchronises with the host.  Samples behind an
utterance's end are never read, and an utterance gives the same bits alone as inside any batch.  The frames are the F0
track's, at the STFT hop, not the 5 ms of most papers.  include/flowtron_hip.h states the rule, tests/envelope_ref.py replays
it in float64.  NOT pinned against pyworld or pysptk (neither was available); two deliberate deviations from WORLD: one
deterministic floor of 1e-20 in place of its two random-noise safeguards, and a directly summed smoothing in place of the
difference of two cumulative sums."""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from . import _lib as L
from .level import _audio_arg, _int_arg, _lengths, _pos_arg, _real_arg

FFT_SIZES = (512, 1024, 2048)
MAX_ORDER = 32             # FT_ENVELOPE_MAX_ORDER (and metrics.MAX_COEFFS: the DTW takes the coefficients as they are)
F0_CEIL = 1000.0
F0_DEFAULT = 500.0
FLOOR = 1e-20
SPTK_ALPHA = {8000: 0.31, 16000: 0.42, 22050: 0.455, 44100: 0.544, 48000: 0.554}


# ---- host tables (float64) ----------------------------------------------------------------------------------------------------------

def fft_size(sampling_rate, f0_floor=71.0):
    """CheapTrick's transform length: 2 ** (1 + floor(log2(3 sr / f0_floor + 1))), the power of two above the widest window.
    512 at 8000 and 11025 Hz, 1024 at 16000 .. 24000, 2048 at 32000 .. 48000 with the default floor; NotImplementedError for
    any other result."""
    sr = _rate_arg(sampling_rate)
    fl = _pos_arg(f0_floor, "f0_floor")
    n = 2 ** (1 + int(math.floor(math.log2(3.0 * sr / fl + 1.0))))
    if n not in FFT_SIZES:
        raise NotImplementedError("fft_size %d (sampling_rate %d, f0_floor %g): the kernels hold 512, 1024 and 2048" % (n, sr, fl))
    return n


def freqt_matrix(H, order, alpha):
    """A [order + 1, H + 1] float64 with freqt(c) = A c for every c of H + 1 coefficients: SPTK's frequency-transform recursion
    (all-pass constant alpha) run over i = H .. 0 on the H + 1 unit vectors at once."""
    a = float(alpha)
    d = np.zeros((order + 1, H + 1))
    g = np.zeros_like(d)
    for i in range(H, -1, -1):
        g[0] = a * d[0]
        g[0, i] += 1.0
        if order >= 1:
            g[1] = (1.0 - a * a) * d[0] + a * d[1]
        for j in range(2, order + 1):
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
        d, g = g, d
    return d


def twiddle_table(n_fft):
    """[3 n_fft / 4, 2] float32: (cos, -sin)(2 pi j / n_fft), formed in float64 and rounded once"""
    j = np.arange(3 * n_fft // 4, dtype=np.float64)
    return np.stack([np.cos(2.0 * np.pi * j / n_fft), -np.sin(2.0 * np.pi * j / n_fft)], axis=1).astype(np.float32)


_TABLES = {}               # ("tw", n_fft, device) / ("freqt", H, order, alpha, device) -> fp32 tensor on the device


def _twiddle(n_fft, dev):
    key = ("tw", n_fft, dev)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(twiddle_table(n_fft)).to(dev)
    return _TABLES[key]


def _freqt(H, order, alpha, dev):
    key = ("freqt", H, order, alpha, dev)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(freqt_matrix(H, order, alpha).astype(np.float32)).to(dev)
    return _TABLES[key]


# ---- argument checks ----------------------------------------------------------------------------------------------------------------

def _rate_arg(sampling_rate):
    if isinstance(sampling_rate, bool) or not isinstance(sampling_rate, numbers.Integral) or not 1 <= sampling_rate <= 1 << 22:
        raise ValueError("sampling_rate must be an integer in 1 ..= %d, got %r" % (1 << 22, sampling_rate))
    return int(sampling_rate)


def _frame_args(sampling_rate, hop_length, f0_floor, q1):
    """-> (sr, hop, f0_floor, q1, n_fft); every refusal that needs no tensor"""
    sr = _rate_arg(sampling_rate)
    hop = _int_arg(hop_length, "hop_length", 1)
    fl = _pos_arg(f0_floor, "f0_floor")
    if fl > F0_CEIL:
        raise ValueError("f0_floor must not exceed %g Hz, got %g" % (F0_CEIL, fl))
    q = _real_arg(q1, "q1")
    n_fft = fft_size(sr, fl)
    if F0_CEIL * n_fft / sr + 2.0 > min(n_fft // 2, 250):
        raise ValueError("sampling_rate %d at fft_size %d: a bin of %.3f Hz is too narrow for the DC correction at %g Hz"
                         % (sr, n_fft, sr / n_fft, F0_CEIL))
    return sr, hop, fl, q, n_fft


def alpha_for(sampling_rate):
    """the customary SPTK all-pass constant for the rate; ValueError where there is none"""
    if sampling_rate not in SPTK_ALPHA:
        raise ValueError("no customary alpha for %r Hz (known: %s): give alpha=" % (sampling_rate, sorted(SPTK_ALPHA)))
    return SPTK_ALPHA[sampling_rate]


def _cepstrum_args(order, alpha, sr, n_fft):
    if isinstance(order, bool) or not isinstance(order, numbers.Integral) or not 1 <= order <= MAX_ORDER:
        raise ValueError("order must be an integer in 1 ..= %d, got %r" % (MAX_ORDER, order))
    if order >= n_fft // 2:
        raise ValueError("order must be below H = %d, got %d" % (n_fft // 2, order))
    if alpha is None:
        a = alpha_for(sr)
    else:
        a = _real_arg(alpha, "alpha")
        if not -1.0 < a < 1.0:
            raise ValueError("alpha must lie inside (-1, 1), got %r" % (alpha,))
    return int(order), a


def _f0_arg(f0, B, T, single):
    if not torch.is_tensor(f0) or f0.dim() not in (1, 2):
        raise ValueError("f0 must be a [T] or [B, T] tensor, got %s" % ((tuple(f0.shape) if torch.is_tensor(f0) else type(f0).__name__),))
    if f0.dtype != torch.float32:
        raise ValueError("f0 must be float32, got %s" % f0.dtype)
    f2 = f0[None] if f0.dim() == 1 else f0
    if f0.dim() == 1 and not single:
        raise ValueError("f0 must be [B, T] for a batch, got shape %s" % (tuple(f0.shape),))
    if f2.shape[0] != B:
        raise ValueError("f0 holds %d contours for %d utterances" % (f2.shape[0], B))
    if f2.shape[1] < T:
        raise ValueError("f0 must hold at least N // hop_length + 1 = %d frames, got %d" % (T, f2.shape[1]))
    return f2.detach()


# ---- the launch ---------------------------------------------------------------------------------------------------------------------

def _launch(a2, n32, f2, sr, hop, fl, q1, n_fft, order, alpha, want_env, want_mc):
    B, N = a2.shape
    T, H = N // hop + 1, n_fft // 2
    dev = a2.device
    env = torch.empty(B, T, H + 1, dtype=torch.float32, device=dev) if want_env else None
    mc = torch.empty(B, T, order + 1, dtype=torch.float32, device=dev) if want_mc else None
    A = _freqt(H, order, alpha, dev) if want_mc else None
    L.check(L.lib().ft_spectral_envelope(L.ptr(a2), *a2.stride(), L.ptr(n32), L.ptr(f2), *f2.stride(), L.ptr(_twiddle(n_fft, dev)),
                                         L.ptr(A), L.ptr(env), L.ptr(mc), B, N, f2.shape[1], hop, n_fft, order if want_mc else 0,
                                         float(np.float32(sr)), float(np.float32(1.5 * sr)), float(np.float32(fl)),
                                         float(np.float32(q1)), L.stream()), "ft_spectral_envelope")
    return env, mc


def _run(audio, n_samples, f0, frame, cep, want_env, who):
    a2, single = _audio_arg(audio, who)
    sr, hop, fl, q1, n_fft = frame
    order, alpha = cep if cep is not None else (0, 0.0)
    B, N = a2.shape
    f2 = _f0_arg(f0, B, N // hop + 1, single)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2, f2)
    env, mc = _launch(a2, n32, f2, sr, hop, fl, q1, n_fft, order, alpha, want_env, cep is not None)
    if single:
        env, mc = (None if env is None else env[0]), (None if mc is None else mc[0])
    return env, mc


# ---- the public calls ---------------------------------------------------------------------------------------------------------------

def spectral_envelope(audio, n_samples, f0, sampling_rate=22050, hop_length=256, f0_floor=71.0, q1=-0.15):
    """The CheapTrick POWER envelope: -> [B, T, H + 1] fp32 ([T, H + 1] for [N]), T = N // hop_length + 1 frames centred on
    samples t * hop_length, H = fft_size(sampling_rate, f0_floor) / 2 bins of sampling_rate / fft_size Hz.  f0 [B, T'] fp32 Hz
    as pitch.f0 / pitch.f0_track return it at this hop (T' >= T, further frames are ignored; ValueError for fewer); a frame
    whose f0 is not inside f0_floor ..= 1000 Hz (unvoiced: 0; NaN, infinite) is analysed at 500 Hz.  Frames behind an
    utterance's own n // hop_length + 1 are zero.  One launch."""
    frame = _frame_args(sampling_rate, hop_length, f0_floor, q1)
    return _run(audio, n_samples, f0, frame, None, True, "spectral_envelope")[0]


def mel_cepstra(audio, n_samples, f0, sampling_rate=22050, hop_length=256, order=24, alpha=None, f0_floor=71.0, q1=-0.15,
                return_envelope=False):
    """Mel-cepstra c0 .. c_order of the CheapTrick envelope: -> [B, T, order + 1] fp32, zero behind an utterance's frames:
    SPTK's frequency transform (all-pass constant alpha; None: the customary value for 8000, 16000, 22050, 44100 or 48000 Hz,
    ValueError at any other rate) of the liftered cepstrum of the log amplitude, which the envelope computation holds anyway:
    the same single launch, and without return_envelope the envelope is neither transformed back nor written.
    return_envelope: -> (mc, env).  1 <= order <= 32, order < H."""
    frame = _frame_args(sampling_rate, hop_length, f0_floor, q1)
    cep = _cepstrum_args(order, alpha, frame[0], frame[4])
    env, mc = _run(audio, n_samples, f0, frame, cep, bool(return_envelope), "mel_cepstra")
    return (mc, env) if return_envelope else mc
