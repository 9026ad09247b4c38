"""Host-side mirror of the reference audio front end (audio_processing.py:96-134, 172-235):
TacotronSTFT.mel_spectrogram as ONE HIP kernel (reflect pad + windowed real FFT in LDS + |X| + sparse mel
filterbank + log-compression) instead of a 1026x1024 dense-DFT conv1d.  Two kernel families share the work
(STFT._call picks one): ft_stft_r8 / ft_istft_r8 (csrc/stft_r8.hip) at n_fft 1024 with hop <= 256, and
ft_stft_pow2 / ft_istft_pow2 (csrc/stft_pow2.hip) at every other setting with n_fft in POW2_NFFT and
1 <= hop <= win_length <= n_fft; both sit on csrc/stft_common.h.  Only a mel spectrogram outside both (n_fft 64 or
128, more than 128 mel channels, a hop above win_length) falls to ft_stft_mel (csrc/stft.hip: complex radix-2 FFT
+ dense filterbank), which takes every power-of-two n_fft from 64 to 4096 with hop <= n_fft whose frames fit its
160 KB of LDS.  Any other n_fft, and a signal no longer than n_fft / 2 (the reflect padding needs more), is
refused by every entry: mel_spectrogram raises.

The synthesis side (audio_processing.py:7-75, 237-270) is here too: STFT.inverse / STFT.forward run
the inverse real FFT + overlap-add kernel of the setting's family, `griffin_lim` loops it with the forward
kernel on the device, and `window_sumsquare` is the reference's host function.  TacotronSTFT.mel_to_magnitude /
mel_to_audio (not in the reference) turn model output into a waveform; the `_ragged` forms (STFT.transform_ragged /
inverse_ragged, `griffin_lim_ragged`, mel_to_magnitude_ragged / mel_to_audio_ragged) do the same for a batch of utterances of
different lengths in one launch per step.  `spsi_phase` (ft_spsi_phase, not in the reference either) is the single-pass
phase start that griffin_lim / mel_to_audio take with phase_init="spsi".

The mel filterbank constants come from librosa in the reference (third-party dependency that is
not vendored: requirements.txt:4 pins 0.6.3, Dockerfile:6 pins 0.8.0; call site
audio_processing.py:104-105 -> htk=False, Slaney area normalisation).  librosa is not installed
here, so `slaney_mel_filterbank` restates the published formula; if librosa IS importable it is
used, exactly like the reference.  PARITY UNPINNED for these constants (no reference test holds them).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from .ops import gemm_raw


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = math.log(6.4) / 27.0
    with np.errstate(divide="ignore"):
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def slaney_mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None) -> np.ndarray:
    """[n_mels, n_fft//2+1] float32 triangular filters, Slaney mel scale, area-normalised."""
    if fmax is None:
        fmax = sr / 2.0
    try:                                         # the reference's own source of these constants, when present
        from librosa.filters import mel as librosa_mel_fn
        return np.asarray(librosa_mel_fn(sr=sr, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax), dtype=np.float32)
    except Exception:
        pass
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    return (w * enorm[:, None]).astype(np.float32)


def hann_window(win_length: int, filter_length: int, dtype=np.float32) -> np.ndarray:
    """scipy.signal.get_window('hann', win_length, fftbins=True) zero-centre-padded to filter_length
    (audio_processing.py:193-197)."""
    n = np.arange(win_length, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
    lpad = (filter_length - win_length) // 2
    out = np.zeros(filter_length, dtype=np.float64)
    out[lpad:lpad + win_length] = w
    return out.astype(dtype)


def window_sumsquare(window, n_frames, hop_length=200, win_length=800, n_fft=800, dtype=np.float32, norm=None):
    """audio_processing.py:7-56 (librosa 0.6): the sum-square envelope of the window at this hop, shape
    [n_fft + hop_length * (n_frames - 1)], on the host.  Only the hann window without normalisation (what STFT uses)."""
    if not (isinstance(window, str) and window == "hann"):
        raise NotImplementedError("window_sumsquare supports window='hann' only, got %r" % (window,))
    if norm is not None:
        raise NotImplementedError("window_sumsquare supports norm=None only, got %r" % (norm,))
    if win_length is None:
        win_length = n_fft
    n = n_fft + hop_length * (n_frames - 1)
    x = np.zeros(n, dtype=dtype)
    win_sq = hann_window(win_length, n_fft, dtype=np.float64) ** 2
    for i in range(n_frames):
        sample = i * hop_length
        x[sample:min(n, sample + n_fft)] += win_sq[:max(0, min(n_fft, n - sample))]
    return x


def _check_momentum(momentum):
    if isinstance(momentum, (bool, np.bool_)) or not isinstance(momentum, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(momentum) < 1.0:
        raise ValueError("momentum must be a number in [0, 1), got %r" % (momentum,))
    return float(momentum)


def _momentum_step(mag_c, angles, prev, nf, momentum, first):
    """The fast Griffin-Lim step on the transform's (magnitude, phase), in place on the phase: one ft_gl_momentum launch."""
    B, nb, T = angles.shape
    L.check(L.lib().ft_gl_momentum(L.ptr(mag_c), L.ptr(angles), L.ptr(prev[0]), L.ptr(prev[1]), L.ptr(nf), B, nb, T, momentum,
                                   1 if first else 0, L.stream()), "ft_gl_momentum")


PHASE_INITS = ("random", "spsi")


def _check_phase_init(phase_init, angles):
    if not isinstance(phase_init, str) or phase_init not in PHASE_INITS:
        raise ValueError("phase_init must be one of %s, got %r" % (PHASE_INITS, phase_init))
    if phase_init != "random" and angles is not None:
        raise ValueError("phase_init=%r computes the starting angles itself: it is refused together with angles=" % phase_init)
    return phase_init


def _spsi_launch(m, nf, stft_fn):
    """m [B, n_fft/2+1, T] contiguous fp32 on the device, nf [B] int32 on the device or None -> angles of m's shape: one
    ft_spsi_phase launch."""
    B, _, T = m.shape
    angles = torch.empty_like(m)
    L.check(L.lib().ft_spsi_phase(L.ptr(m), L.ptr(angles), L.ptr(nf), B, stft_fn.filter_length, stft_fn.hop_length, T, L.stream()),
            "ft_spsi_phase")
    return angles


def spsi_phase(magnitudes, stft_fn, n_frames=None):
    """Single Pass Spectrogram Inversion (Beauregard, Harish, Wyse 2015; not in the reference): a starting phase for Griffin-Lim
    from the magnitudes alone, in one launch (ft_spsi_phase, csrc/vocode.hip; the rule is in include/flowtron_hip.h).  Every
    frame's spectral peaks get an instantaneous frequency by quadratic interpolation, a per-bin accumulator advances by
    hop x frequency from frame to frame, and the bins of a peak's lobe are locked to the peak's phase.
    magnitudes [B, n_fft/2+1, T] or [n_fft/2+1, T] float32 on the device, stft_fn an STFT with a device path; n_frames (host
    integers in 0 ..= T, one per utterance): the batch is ragged, the angles at and behind an utterance's end are 0 and the
    magnitudes there are never read.  Returns float32 angles of the magnitudes' shape in [-pi, pi]."""
    stft_fn._require_device_path("spsi_phase")
    nb = stft_fn.filter_length // 2 + 1
    if not torch.is_tensor(magnitudes) or magnitudes.dim() not in (2, 3) or magnitudes.shape[-2] != nb or magnitudes.shape[-1] < 1:
        raise ValueError("spsi_phase needs magnitudes of shape [B, %d, T] or [%d, T] with T >= 1, got %s"
                         % (nb, nb, tuple(magnitudes.shape) if torch.is_tensor(magnitudes) else type(magnitudes).__name__))
    if magnitudes.dtype != torch.float32:
        raise ValueError("spsi_phase needs float32 magnitudes, got %s" % magnitudes.dtype)
    m = magnitudes if magnitudes.dim() == 3 else magnitudes[None]
    B, _, T = m.shape
    lens = None if n_frames is None else _host_lengths(n_frames, B, 0, T, "n_frames", "0 ..= T = %d" % T)
    L.require_cuda(magnitudes)
    m = m.contiguous()
    angles = _spsi_launch(m, None if lens is None else _lengths_to_device(lens, m.device), stft_fn)
    return angles if magnitudes.dim() == 3 else angles[0]


def griffin_lim(magnitudes, stft_fn, n_iters=30, momentum=0.0, n_frames=None, angles=None, phase_init="random"):
    """audio_processing.py:59-75 on the device.  magnitudes [B, n_fft/2+1, T] (device tensor), stft_fn an STFT.
    The starting angles are drawn on the host exactly as the reference draws them (np.random.rand, so np.random.seed(s)
    gives the reference's starting point) and copied to the device once; then n_iters x (ft_stft_r8 for the phase +
    ft_istft_r8, or ft_stft_pow2 + ft_istft_pow2 off the 1024 setting) run without a host synchronisation.
    momentum (not in the reference; 0 <= momentum < 1) > 0 is fast Griffin-Lim (Perraudin et al. 2013; the common Python audio
    library runs it at 0.99): with c the transform of an iteration's signal, the next phase is that of c + momentum (c - c_prev)
    (ft_gl_momentum, one more launch per iteration between the two, the two planes of c_prev allocated once); the first
    iteration has no c_prev and is the plain one, so n_iters = 1 gives the same bits with and without it.
    n_frames (host integers, one per utterance; not in the reference): the batch is ragged and goes through griffin_lim_ragged's
    loop with this momentum (1 + 3 n_iters launches for the whole batch when momentum > 0), from `angles` when given;
    griffin_lim_ragged itself keeps its signature and is that loop at momentum 0.
    phase_init (not in the reference): "random" is the draw above; "spsi" starts from spsi_phase(magnitudes) instead (one more
    launch, no draw, refused together with angles=) and runs the ragged loop, a dense batch with every length T.  From that
    start a few iterations do what some thirty do from the random one, and n_iters = 0 is the single-pass inversion.
    Returns [B, hop * (T - 1)]."""
    momentum = _check_momentum(momentum)
    phase_init = _check_phase_init(phase_init, angles)
    if n_frames is not None or phase_init != "random":
        return _griffin_lim_ragged(magnitudes, n_frames, stft_fn, n_iters, angles, momentum, phase_init)
    if angles is not None:
        raise ValueError("griffin_lim takes starting angles only with n_frames (the dense call draws them as the reference does)")
    L.require_cuda(magnitudes)
    stft_fn._check_spectrum(magnitudes, magnitudes)
    T = magnitudes.shape[-1]
    if stft_fn.hop_length * (T - 1) <= stft_fn.filter_length // 2:
        raise ValueError("griffin_lim needs hop * (T - 1) > filter_length / 2 samples for the reflect padding of STFT.transform; "
                         "got T = %d frames at hop %d" % (T, stft_fn.hop_length))
    angles = np.angle(np.exp(2j * np.pi * np.random.rand(*magnitudes.size())))
    angles = torch.from_numpy(angles.astype(np.float32)).to(magnitudes.device)
    signal = stft_fn.inverse(magnitudes, angles).squeeze(1)
    prev = torch.empty((2,) + tuple(magnitudes.shape), device=magnitudes.device, dtype=torch.float32) \
        if momentum > 0.0 and n_iters > 0 else None
    for it in range(n_iters):
        mag_c, angles = stft_fn.transform(signal)
        if prev is not None:
            _momentum_step(mag_c, angles, prev, None, momentum, it == 0)
        signal = stft_fn.inverse(magnitudes, angles).squeeze(1)
    return signal


def _host_lengths(lengths, B, lo, hi, name, rule):
    """The per-utterance lengths of a ragged batch as a list of B Python ints in lo ..= hi: a list, a tuple or a CPU integer
    tensor (what Flowtron.infer(..., return_lengths=True) hands back).  ValueError names the argument and the utterance."""
    if torch.is_tensor(lengths):
        if lengths.is_cuda or lengths.dim() != 1 or lengths.is_floating_point() or lengths.is_complex() \
                or lengths.dtype == torch.bool:
            raise ValueError("%s must be host integers (a list, a tuple or a 1-D CPU integer tensor), got a %s %s tensor of shape %s"
                             % (name, lengths.device.type, lengths.dtype, tuple(lengths.shape)))
        lengths = lengths.tolist()
    elif isinstance(lengths, np.ndarray):
        lengths = lengths.tolist()
    elif not isinstance(lengths, (list, tuple)):
        raise ValueError("%s must be host integers (a list, a tuple or a 1-D CPU integer tensor), got %s"
                         % (name, type(lengths).__name__))
    if len(lengths) != B:
        raise ValueError("%s holds %d lengths for a batch of %d utterances" % (name, len(lengths), B))
    out = []
    for b, n in enumerate(lengths):
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
            raise ValueError("%s[%d] = %r is not an integer" % (name, b, n))
        if not lo <= n <= hi:
            raise ValueError("%s[%d] = %d is outside %s" % (name, b, n, rule))
        out.append(int(n))
    return out


def _check_reflect(lens, stft_fn, what, name):
    """griffin_lim's rule for every utterance of a ragged batch: its own samples must outnumber the reflect padding."""
    for b, n in enumerate(lens):
        if stft_fn.hop_length * (n - 1) <= stft_fn.filter_length // 2:
            raise ValueError("%s needs hop * (%s[b] - 1) > filter_length / 2 samples for the reflect padding of STFT.transform; "
                             "got %s[%d] = %d frames at hop %d" % (what, name, name, b, n, stft_fn.hop_length))


def _lengths_to_device(values, device):
    """Host ints -> int32 on the device through pinned memory, without blocking the host (as Flowtron.infer_batch does)."""
    return torch.tensor(values, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def griffin_lim_ragged(magnitudes, n_frames, stft_fn, n_iters=30, angles=None):
    """griffin_lim for a batch of utterances of different lengths in one pass: magnitudes [B, n_fft/2+1, T] (device tensor),
    utterance b holds n_frames[b] <= T frames (host integers); frames behind that may hold anything, they are never read.
    Returns [B, hop * (T - 1)]: utterance b occupies [: hop * (n_frames[b] - 1)] and equals griffin_lim on its own frames from
    the same starting angles, zeros behind.  angles=None draws np.random.rand(*magnitudes.size()) exactly as griffin_lim does
    (with every length = T the two start from the same point under one seed); otherwise a [B, n_fft/2+1, T] starting phase on
    the host or the device.  The lengths go to the device once; then 1 + 2 n_iters launches (ft_istft_*_ragged, and
    ft_stft_*_ragged_phase storing the phase only) serve the whole batch without a host synchronisation.
    The fast iteration of a ragged batch is griffin_lim(..., momentum=, n_frames=, angles=): 1 + 3 n_iters launches (the
    analysis launch stores the magnitude too and ft_gl_momentum follows it); cells behind an utterance's end are neither read
    nor written, so the promise above holds there as well."""
    return _griffin_lim_ragged(magnitudes, n_frames, stft_fn, n_iters, angles, 0.0)


def _griffin_lim_ragged(magnitudes, n_frames, stft_fn, n_iters, angles, momentum, phase_init="random"):
    """The body of griffin_lim_ragged, with griffin_lim's momentum and phase_init (n_frames None: every utterance T frames)."""
    L.require_cuda(magnitudes)
    stft_fn._check_spectrum(magnitudes, magnitudes)
    B, nb, T = magnitudes.shape
    hop = stft_fn.hop_length
    lens = [T] * B if n_frames is None else _host_lengths(n_frames, B, 1, T, "n_frames", "1 ..= T = %d" % T)
    _check_reflect(lens, stft_fn, "griffin_lim_ragged", "n_frames")
    if phase_init == "spsi":
        pass                                            # from the magnitudes, once they and the lengths are on the device
    elif angles is None:
        angles = np.angle(np.exp(2j * np.pi * np.random.rand(*magnitudes.size())))
        angles = torch.from_numpy(angles.astype(np.float32))
    else:
        angles = torch.as_tensor(angles)
        if tuple(angles.shape) != (B, nb, T):
            raise ValueError("griffin_lim_ragged needs angles of the magnitudes' shape %s, got %s"
                             % ((B, nb, T), tuple(angles.shape)))
    m = magnitudes.contiguous().float()
    if stft_fn.fft_window.device != m.device:
        stft_fn.to(m.device)
    both = _lengths_to_device(lens + [hop * (n - 1) for n in lens], m.device)
    nf, ns = both[:B], both[B:]
    if phase_init == "spsi":
        angles = _spsi_launch(m, nf, stft_fn)
    else:
        angles = angles.to(magnitudes.device, torch.float32).contiguous()
    signal = stft_fn._inverse_ragged(m, angles, nf)
    prev = torch.empty((2, B, nb, T), device=m.device, dtype=torch.float32) if momentum > 0.0 and n_iters > 0 else None
    for it in range(n_iters):
        mag_c, angles = stft_fn._transform_ragged(signal, ns, want_magnitude=prev is not None)
        if prev is not None:
            _momentum_step(mag_c, angles, prev, nf, momentum, it == 0)
        signal = stft_fn._inverse_ragged(m, angles, nf)
    return signal


RESAMPLE_WIDTH = 6           # zero crossings of the sinc kept on each side (the common torch audio library's lowpass_filter_width)
RESAMPLE_RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)      # every ordered pair of these fits the kernel's table
_RESAMPLE_HOST = {}          # (orig, new) -> (taps [new_g, K] fp32, phase_start [new_g] int32, orig_g, new_g, K)
_RESAMPLE_DEV = {}           # (orig, new, device) -> (taps, phase_start) on the device


def _check_rates(orig_sr, new_sr):
    for name, r in (("orig_sr", orig_sr), ("new_sr", new_sr)):
        if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, np.integer)) or r < 1:
            raise ValueError("%s must be a positive integer number of Hz, got %r" % (name, r))
    return int(orig_sr), int(new_sr)


def resample_length(n, orig_sr, new_sr):
    """Samples `resample` returns for n samples: ceil(n * new_sr / orig_sr), host integer arithmetic only."""
    orig, new = _check_rates(orig_sr, new_sr)
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError("n must be a non-negative integer, got %r" % (n,))
    return (int(n) * new + orig - 1) // orig


def resample_taps(orig_sr, new_sr):
    """The polyphase table of the Hann-windowed sinc (width RESAMPLE_WIDTH, rolloff 0.99) for orig_sr -> new_sr, built once per
    pair in float64 and rounded to fp32: (taps [new_g, K], phase_start [new_g] int32, orig_g, new_g, K) with g = gcd,
    orig_g = orig_sr / g, new_g = new_sr / g.  Output m = q new_g + p is sum_i taps[p, i] x[q orig_g + phase_start[p] + i], where
    taps[p, i] = h((phase_start[p] + i) / orig_sr - p / new_sr), h(t) = (base / orig_sr) sinc(base t) cos^2(pi base t / (2 W))
    inside |base t| < W, base = 0.99 min(orig_sr, new_sr).  The argument base t is formed from the exact integer
    k new_sr - m orig_sr, so the table does not depend on which output of a phase it is evaluated at."""
    orig, new = _check_rates(orig_sr, new_sr)
    hit = _RESAMPLE_HOST.get((orig, new))
    if hit is not None:
        return hit
    g = math.gcd(orig, new)
    og, ng = orig // g, new // g
    mn, W = min(orig, new), RESAMPLE_WIDTH
    # |base t| < W  <=>  99 mn |num| < 100 W orig new  with  num = k new - m orig = g (j ng - p og),  j = k - q og
    u_max = (100 * W * orig * new - 1) // (99 * mn * g)                  # largest |j ng - p og| inside the window
    K = 2 * u_max // ng + 2                                              # no phase has more taps than this
    if ng <= L.RESAMPLE_MAX_PHASES:
        K = max((p * og + u_max) // ng + (u_max - p * og) // ng + 1 for p in range(ng))
    if ng > L.RESAMPLE_MAX_PHASES or ng * K > L.RESAMPLE_MAX_TAPS:
        raise NotImplementedError(
            "resample %d -> %d Hz needs a table of %d phases x %d taps; the kernel holds at most %d phases and %d taps in all "
            "(supported: every ordered pair of %s Hz, and any pair whose rates share a large enough common divisor)"
            % (orig, new, ng, K, L.RESAMPLE_MAX_PHASES, L.RESAMPLE_MAX_TAPS, "/".join(map(str, RESAMPLE_RATES))))
    taps = np.zeros((ng, K), dtype=np.float64)
    start = np.zeros(ng, dtype=np.int32)
    base = 0.99 * mn
    for p in range(ng):
        j_lo, j_hi = -((u_max - p * og) // ng), (p * og + u_max) // ng
        start[p] = j_lo
        for j in range(j_lo, j_hi + 1):
            t = base * (g * (j * ng - p * og)) / (orig * new)
            s = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
            taps[p, j - j_lo] = (base / orig) * s * math.cos(math.pi * t / (2 * W)) ** 2
    # the kernel sizes a tile's input span from these two facts (include/flowtron_hip.h)
    assert np.all(np.diff(start) >= 0) and int(start[-1]) <= int(start[0]) + og
    out = _RESAMPLE_HOST[(orig, new)] = (taps.astype(np.float32), start, og, ng, K)
    return out


def _resample_launch(x, ns_dev, orig, new, n_out_max):
    """x [B, N] contiguous fp32 on the device, ns_dev int32 [B] on the device or None (every row N long) -> [B, n_out_max]:
    one ft_resample_ragged launch."""
    taps, start, og, ng, K = resample_taps(orig, new)
    key = (orig, new, str(x.device))
    dev = _RESAMPLE_DEV.get(key)
    if dev is None:
        dev = _RESAMPLE_DEV[key] = (torch.from_numpy(taps).to(x.device), torch.from_numpy(start).to(x.device))
    B, N = x.shape
    y = torch.empty(B, n_out_max, device=x.device, dtype=torch.float32)
    L.check(L.lib().ft_resample_ragged(L.ptr(x), L.ptr(ns_dev), L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(y), B, N, n_out_max, og, ng, K,
                                       L.stream()), "ft_resample_ragged")
    return y


def resample(audio, orig_sr, new_sr):
    """Bandlimited sample-rate conversion on the device (ft_resample_ragged, csrc/resample.hip): audio [N] or [B, N] at orig_sr
    -> [n_out] or [B, n_out] at new_sr, n_out = resample_length(N, orig_sr, new_sr).  The filter is the Hann-windowed sinc the
    common torch audio library uses at its defaults (lowpass_filter_width 6, rolloff 0.99); samples outside the signal count
    as zero.  Equal rates return the input's values without a launch.  Rates: positive integers whose table fits the kernel
    (every ordered pair of RESAMPLE_RATES does), NotImplementedError otherwise."""
    orig, new = _check_rates(orig_sr, new_sr)
    if not torch.is_tensor(audio) or audio.dim() not in (1, 2) or audio.shape[-1] < 1:
        raise ValueError("resample needs audio of shape [N] or [B, N] with N >= 1, got %s"
                         % (tuple(audio.shape) if torch.is_tensor(audio) else type(audio).__name__,))
    if orig != new:
        resample_taps(orig, new)
    L.require_cuda(audio)
    x = audio.contiguous().float()
    if orig == new:
        return x
    x2 = x if x.dim() == 2 else x[None]
    y = _resample_launch(x2, None, orig, new, resample_length(x2.shape[1], orig, new))
    return y if x.dim() == 2 else y[0]


def resample_ragged(audio, n_samples, orig_sr, new_sr):
    """resample for a zero-padded batch of utterances of different lengths in one launch: audio [B, N] on the device, utterance b
    holds n_samples[b] samples (host integers, 1 ..= N; the samples behind them are never read) -> (out [B, max_b n_out[b]],
    n_out int64 CPU [B]) with n_out[b] = resample_length(n_samples[b], orig_sr, new_sr): out[b, :n_out[b]] equals
    resample(audio[b, :n_samples[b]], ...) bit for bit, zeros behind."""
    orig, new = _check_rates(orig_sr, new_sr)
    if not torch.is_tensor(audio) or audio.dim() != 2 or audio.shape[1] < 1:
        raise ValueError("resample_ragged needs audio of shape [B, N] with N >= 1, got %s"
                         % (tuple(audio.shape) if torch.is_tensor(audio) else type(audio).__name__,))
    B, N = audio.shape
    lens = _host_lengths(n_samples, B, 1, N, "n_samples", "1 ..= N = %d" % N)
    if orig != new:
        resample_taps(orig, new)
    L.require_cuda(audio)
    x = audio.contiguous().float()
    n_out = [resample_length(n, orig, new) for n in lens]
    if orig == new:
        behind = torch.arange(N, device=x.device)[None, :] >= _lengths_to_device(lens, x.device)[:, None]
        return x.masked_fill(behind, 0.0)[:, :max(lens)], torch.tensor(n_out, dtype=torch.int64)
    y = _resample_launch(x, _lengths_to_device(lens, x.device), orig, new, max(n_out))
    return y, torch.tensor(n_out, dtype=torch.int64)


def dynamic_range_compression(x, C=1, clip_val=1e-5):
    return torch.log(torch.clamp(x, min=clip_val) * C)


def dynamic_range_decompression(x, C=1):
    return torch.exp(x) / C


def filterbank_csr(mel_basis: np.ndarray):
    """[n_mel, n_bins] triangular filterbank -> (first bin per band int32[n_mel], row pointer int32[n_mel+1], weights fp32[nnz]):
    every band's non-zeros are one run of consecutive bins (a triangle), ~1 000 weights instead of 80 x 513."""
    bin0, ptr, w = [], [0], []
    for row in np.asarray(mel_basis, dtype=np.float32):
        nz = np.nonzero(row)[0]
        if len(nz) == 0:
            bin0.append(0)
            ptr.append(ptr[-1])
            continue
        bin0.append(int(nz[0]))
        w.extend(row[nz[0]:nz[-1] + 1].tolist())
        ptr.append(len(w))
    return np.asarray(bin0, np.int32), np.asarray(ptr, np.int32), np.asarray(w, np.float32)


def filterbank_bin_table(bin0, ptr, w, n_bins):
    """The transpose of filterbank_csr's bands, per bin: (band int32 [n_bins, 2], weight fp32 [n_bins, 2]) = the bands whose
    run holds the bin, lower band first, -1 / 0 where there is none.  Slaney triangles overlap at most pairwise; a bin in more
    than two bands raises NotImplementedError (ft_mel_nnls holds two per bin)."""
    band = np.full((n_bins, 2), -1, dtype=np.int32)
    weight = np.zeros((n_bins, 2), dtype=np.float32)
    count = np.zeros(n_bins, dtype=np.int64)
    for j in range(len(bin0)):
        for i in range(int(ptr[j + 1] - ptr[j])):
            k = int(bin0[j]) + i
            if count[k] == 2:
                raise NotImplementedError("bin %d of the mel filterbank lies in more than two bands (band %d is the third); "
                                          "the NNLS mel inversion takes filterbanks whose bands overlap at most pairwise" % (k, j))
            band[k, count[k]] = j
            weight[k, count[k]] = w[ptr[j] + i]
            count[k] += 1
    return band, weight


MEL_INVERSIONS = ("pinv", "nnls")


def _check_inversion(method, n_iters):
    if method not in MEL_INVERSIONS:
        raise ValueError("the mel inversion method must be one of %s, got %r" % (MEL_INVERSIONS, method))
    if isinstance(n_iters, (bool, np.bool_)) or not isinstance(n_iters, (int, np.integer)) or n_iters < 0:
        raise ValueError("the mel inversion takes a non-negative integer number of iterations, got %r" % (n_iters,))


POW2_NFFT = (256, 512, 1024, 2048, 4096)      # the analysis sizes of csrc/stft_pow2.hip


class STFT(torch.nn.Module):
    """The reference STFT (audio_processing.py:172-270): `transform(y)` -> (magnitude, phase), both [B, n_fft/2+1, N // hop + 1]
    (real FFT), `inverse(magnitude, phase)` -> [B, 1, hop * (T - 1)] (inverse real FFT + overlap-add) and `forward(y)` =
    inverse(transform(y)); one HIP kernel each.  fast_path(): n_fft 1024, hop <= 256 (ft_stft_r8 / ft_istft_r8,
    csrc/stft_r8.hip); pow2_path(): every other n_fft in POW2_NFFT with 1 <= hop <= win_length <= n_fft (ft_stft_pow2 /
    ft_istft_pow2, csrc/stft_pow2.hip); any other setting raises NotImplementedError."""

    def __init__(self, filter_length=800, hop_length=200, win_length=800, window="hann"):
        super().__init__()
        assert window == "hann" and filter_length >= win_length
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        self.register_buffer("fft_window", torch.from_numpy(hann_window(win_length, filter_length)))

    def fast_path(self):
        return self.filter_length == 1024 and self.hop_length <= 256

    def pow2_path(self):
        """The settings the power-of-two kernels (csrc/stft_pow2.hip) take that fast_path() does not: n_fft in POW2_NFFT and
        1 <= hop <= win_length <= n_fft."""
        return (not self.fast_path() and self.filter_length in POW2_NFFT
                and 1 <= self.hop_length <= self.win_length <= self.filter_length)

    def _require_device_path(self, what):
        if not (self.fast_path() or self.pow2_path()):
            raise NotImplementedError(
                "%s runs on the device for filter_length in %s with 1 <= hop_length <= win_length <= filter_length (and for "
                "filter_length 1024 with any hop_length <= 256); got filter_length %d, hop_length %d, win_length %d"
                % (what, "/".join(map(str, POW2_NFFT)), self.filter_length, self.hop_length, self.win_length))

    def _call(self, base, tail, head, rest=()):
        """The one place that knows the two kernel families: calls ft_<base>_r8<tail>(*head, hop, *rest, stream) on
        fast_path() and ft_<base>_pow2<tail>(*head, n_fft, hop, win_length, *rest, stream) otherwise, looked up on the
        library by name at call time."""
        if self.fast_path():
            name, geometry = "ft_%s_r8%s" % (base, tail), (self.hop_length,)
        else:
            name, geometry = "ft_%s_pow2%s" % (base, tail), (self.filter_length, self.hop_length, self.win_length)
        L.check(getattr(L.lib(), name)(*head, *geometry, *rest, L.stream()), name)

    def transform(self, input_data):
        """audio_processing.py:207-235."""
        L.require_cuda(input_data)
        self._require_device_path("STFT.transform")
        y = input_data.contiguous().float()
        if self.fft_window.device != y.device:
            self.to(y.device)
        B, N = y.shape
        n_frames = N // self.hop_length + 1
        mag = torch.empty(B, self.filter_length // 2 + 1, n_frames, device=y.device, dtype=torch.float32)
        phase = torch.empty_like(mag)
        self._call("stft", "", (L.ptr(y), L.ptr(self.fft_window), None, None, None, None, L.ptr(mag), L.ptr(phase), B, N), (0,))
        return mag, phase

    def _check_spectrum(self, magnitude, phase):
        self._require_device_path("STFT.inverse")
        nb = self.filter_length // 2 + 1
        if magnitude.dim() != 3 or magnitude.shape[1] != nb or phase.shape != magnitude.shape:
            raise ValueError("STFT.inverse needs magnitude and phase of one shape [B, %d, T], got %s and %s"
                             % (nb, tuple(magnitude.shape), tuple(phase.shape)))

    def inverse(self, magnitude, phase):
        """audio_processing.py:237-263: [B, n_fft/2+1, T] x 2 -> [B, 1, hop * (T - 1)] (ft_istft_r8 / ft_istft_pow2)."""
        L.require_cuda(magnitude, phase)
        self._check_spectrum(magnitude, phase)
        m, ph = magnitude.contiguous().float(), phase.contiguous().float()
        if self.fft_window.device != m.device:
            self.to(m.device)
        B, _, T = m.shape
        y = torch.empty(B, 1, self.hop_length * max(T - 1, 0), device=m.device, dtype=torch.float32)
        if T >= 2:                                      # one frame leaves nothing after the two n_fft/2-sample trims
            self._call("istft", "", (L.ptr(m), L.ptr(ph), L.ptr(self.fft_window), L.ptr(y), B, T))
        return y

    def _transform_ragged(self, y, ns, want_magnitude=True):
        """y [B,N] contiguous fp32, ns [B] int32 on the device -> (magnitude or None, phase): one launch."""
        B, N = y.shape
        phase = torch.empty(B, self.filter_length // 2 + 1, N // self.hop_length + 1, device=y.device, dtype=torch.float32)
        mag = torch.empty_like(phase) if want_magnitude else None
        self._call("stft", "_ragged_phase", (L.ptr(y), L.ptr(ns), L.ptr(self.fft_window), L.ptr(mag), L.ptr(phase), B, N))
        return mag, phase

    def transform_ragged(self, input_data, n_samples):
        """transform for a zero-padded batch in one launch (ft_stft_r8_ragged_phase / ft_stft_pow2_ragged_phase): y [B,N] on the
        device, utterance b holds n_samples[b] samples (host integers, n_fft/2 < n <= N) -> (magnitude, phase), each
        [B, n_fft/2+1, N // hop + 1]: frames t < n_samples[b] // hop + 1 equal transform(y[b:b+1, :n_samples[b]]) (the reflect
        padding is about the utterance's own end, the samples behind it are never read), later frames are zero."""
        L.require_cuda(input_data)
        self._require_device_path("STFT.transform_ragged")
        if input_data.dim() != 2:
            raise ValueError("STFT.transform_ragged needs y of shape [B, N], got %s" % (tuple(input_data.shape),))
        y = input_data.contiguous().float()
        B, N = y.shape
        half = self.filter_length // 2
        lens = _host_lengths(n_samples, B, half + 1, N, "n_samples", "filter_length / 2 = %d < n <= N = %d" % (half, N))
        if self.fft_window.device != y.device:
            self.to(y.device)
        return self._transform_ragged(y, _lengths_to_device(lens, y.device))

    def _inverse_ragged(self, m, ph, nf):
        """m, ph [B, n_fft/2+1, T] contiguous fp32, nf [B] int32 on the device -> [B, hop * (T - 1)]: one launch."""
        B, _, T = m.shape
        y = torch.empty(B, self.hop_length * max(T - 1, 0), device=m.device, dtype=torch.float32)
        if T >= 2:                                      # one frame leaves nothing after the two n_fft/2-sample trims
            self._call("istft", "_ragged", (L.ptr(m), L.ptr(ph), L.ptr(nf), L.ptr(self.fft_window), L.ptr(y), B, T))
        return y

    def inverse_ragged(self, magnitude, phase, n_frames):
        """inverse for a batch of utterances of different lengths in one launch (ft_istft_r8_ragged / ft_istft_pow2_ragged):
        [B, n_fft/2+1, T] x 2 on the device, utterance b holds n_frames[b] frames (host integers, 1 ..= T) ->
        [B, 1, hop * (T - 1)]: the samples [: hop * (n_frames[b] - 1)] equal inverse(magnitude[b:b+1, :, :n_frames[b]], ...),
        zeros behind; the frames t >= n_frames[b] are never read."""
        L.require_cuda(magnitude, phase)
        self._check_spectrum(magnitude, phase)
        m, ph = magnitude.contiguous().float(), phase.contiguous().float()
        B, _, T = m.shape
        lens = _host_lengths(n_frames, B, 1, T, "n_frames", "1 ..= T = %d" % T)
        if self.fft_window.device != m.device:
            self.to(m.device)
        return self._inverse_ragged(m, ph, _lengths_to_device(lens, m.device)).unsqueeze(1)

    def forward(self, input_data):
        """audio_processing.py:265-268."""
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)


class TacotronSTFT(torch.nn.Module):
    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, sampling_rate=22050,
                 mel_fmin=0.0, mel_fmax=None):
        super().__init__()
        self.n_mel_channels = n_mel_channels
        self.sampling_rate = sampling_rate
        self.stft_fn = STFT(filter_length, hop_length, win_length)
        basis = slaney_mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)
        self.register_buffer("mel_basis", torch.from_numpy(basis).float())
        bin0, ptr, w = filterbank_csr(basis)          # sparse form of the same matrix for the rFFT kernel (not in the state_dict)
        self._fb_host = (bin0, ptr, w)                # kept on the host for the per-bin table of the NNLS inversion
        self.register_buffer("fb_bin0", torch.from_numpy(bin0), persistent=False)
        self.register_buffer("fb_ptr", torch.from_numpy(ptr), persistent=False)
        self.register_buffer("fb_w", torch.from_numpy(w), persistent=False)
        # pseudo-inverse of the filterbank for mel_to_magnitude, in float64 once (not in the state_dict)
        self.register_buffer("mel_pinv", torch.from_numpy(np.linalg.pinv(basis.astype(np.float64)).astype(np.float32)),
                             persistent=False)

    def spectral_normalize(self, magnitudes):
        return dynamic_range_compression(magnitudes)

    def spectral_de_normalize(self, magnitudes):
        return dynamic_range_decompression(magnitudes)

    def mel_spectrogram_ragged(self, y, n_samples, max_t=None):
        """The collated batch of the data path in one launch (ft_stft_r8_ragged / ft_stft_pow2_ragged): y [B,N] zero-padded audio on the device,
        n_samples [B] (int32, device) -> [B, n_mel_channels, max_t]; utterance b's frames t < n_samples[b] // hop + 1 equal
        mel_spectrogram(y[b:b+1, :n_samples[b]]), later frames are zero (DataCollate's padding, data.py:215-229).
        The lengths stay on the device, so an utterance of n_samples[b] <= n_fft / 2, which mel_spectrogram refuses, cannot be
        refused here: its n_samples[b] // hop + 1 frames are computed under the kernel's own padding rule, one reflection at
        each end (n < 0 -> -n, then n >= n_samples[b] -> 2 (n_samples[b] - 1) - n) and zeros where the index still falls
        outside the utterance; the other utterances of the batch are not affected."""
        L.require_cuda(y, n_samples)
        y = y.contiguous().float()
        if self.mel_basis.device != y.device:
            self.to(y.device)
        B, N = y.shape
        st = self.stft_fn
        T_out = N // st.hop_length + 1 if max_t is None else int(max_t)
        if not (self.ragged_path() and N > st.filter_length // 2):
            raise NotImplementedError("the ragged front end is built for n_mel_channels <= 128 and n_fft = 1024 with hop <= 256, "
                                      "or n_fft in %s with 1 <= hop <= win_length <= n_fft" % (POW2_NFFT,))
        mel = torch.empty(B, self.n_mel_channels, T_out, device=y.device, dtype=torch.float32)
        ns = n_samples.to(torch.int32)
        st._call("stft", "_ragged", (L.ptr(y), L.ptr(ns), L.ptr(st.fft_window), L.ptr(self.fb_bin0), L.ptr(self.fb_ptr),
                                     L.ptr(self.fb_w), L.ptr(mel), B, N), (self.n_mel_channels, T_out))
        return mel

    def ragged_path(self):
        """True when mel_spectrogram_ragged (one launch per batch) takes this setting: the rFFT kernels of fast_path() or
        pow2_path() with n_mel_channels <= 128."""
        return (self.stft_fn.fast_path() or self.stft_fn.pow2_path()) and self.n_mel_channels <= 128

    def mel_spectrogram(self, y):
        """y [B,N] float32 in [-1,1] (device tensor) -> [B, n_mel_channels, N // hop + 1]."""
        L.require_cuda(y)
        assert y.dim() == 2
        # the reference asserts the value range with two host syncs (audio_processing.py:127-128); done only when the caller asks
        # (TacotronSTFT.check_audio_range = True), to keep the front end sync-free
        if getattr(self, "check_audio_range", False):
            assert float(y.min()) >= -1 and float(y.max()) <= 1
        y = y.contiguous().float()
        if self.mel_basis.device != y.device:
            self.to(y.device)
        B, N = y.shape
        st = self.stft_fn
        n_frames = N // st.hop_length + 1
        mel = torch.empty(B, self.n_mel_channels, n_frames, device=y.device, dtype=torch.float32)
        if self.ragged_path() and N > st.filter_length // 2:
            # rFFT (n_fft/2-point complex FFT + split) + sparse triangular filterbank, one wave per frame (csrc/stft_r8.hip at
            # 1024 with hop <= 256, csrc/stft_pow2.hip at the other power-of-two settings); mel_spectrogram_ragged shares it
            st._call("stft", "", (L.ptr(y), L.ptr(st.fft_window), L.ptr(self.fb_bin0), L.ptr(self.fb_ptr), L.ptr(self.fb_w),
                                  L.ptr(mel), None, None, B, N), (self.n_mel_channels,))
        else:                                           # outside both: complex radix-2 FFT + dense filterbank (csrc/stft.hip)
            L.check(L.lib().ft_stft_mel(L.ptr(y), L.ptr(st.fft_window), L.ptr(self.mel_basis), L.ptr(mel), B, N,
                                        st.filter_length, st.hop_length, self.n_mel_channels, L.stream()), "ft_stft_mel")
        return mel

    def _bin_table(self, device):
        """filterbank_bin_table of this filterbank on `device`, built on the first NNLS inversion and kept."""
        hit = getattr(self, "_bin_table_dev", None)
        if hit is None or hit[0].device != device:
            band, weight = filterbank_bin_table(*self._fb_host, self.mel_pinv.shape[0])
            hit = self._bin_table_dev = (torch.from_numpy(band).to(device), torch.from_numpy(weight).to(device))
        return hit

    def _mel_to_magnitude(self, mel, method, n_iters, lens, what):
        """The body of mel_to_magnitude(_ragged): lens None (dense) or B host integers."""
        if self.mel_pinv.device != mel.device:
            self.to(mel.device)
        if method == "nnls":
            if self.fb_w.numel() < 1:
                raise NotImplementedError("%s: the mel filterbank is empty" % what)
            table = self._bin_table(mel.device)
        x = self.spectral_de_normalize(mel.float()).contiguous()
        x3 = x if x.dim() == 3 else x[None]
        B, n_mel, T = x3.shape
        nb = self.mel_pinv.shape[0]
        out = torch.empty(B, nb, T, device=mel.device, dtype=torch.float32)
        gemm_raw(self.mel_pinv, x3, out, nb, T, n_mel, n_mel, 1, T, 1, T, act=L.ACT_RELU, batch=B, bsA=0, bsB=n_mel * T,
                 bsC=nb * T, mode=L.FT_F32)
        nf = None if lens is None else _lengths_to_device(lens, out.device)
        if method == "nnls":                            # in place on the estimate; zeros behind every length
            L.check(L.lib().ft_mel_nnls(L.ptr(x3), L.ptr(out), L.ptr(out), L.ptr(nf), L.ptr(self.fb_bin0), L.ptr(self.fb_ptr),
                                        L.ptr(self.fb_w), L.ptr(table[0]), L.ptr(table[1]), B, n_mel, self.stft_fn.filter_length, T,
                                        self.fb_w.numel(), int(n_iters), L.stream()), "ft_mel_nnls")
        elif nf is not None:
            out.masked_fill_(torch.arange(T, device=out.device)[None, None, :] >= nf[:, None, None], 0.0)
        return out if mel.dim() == 3 else out[0]

    def mel_to_magnitude(self, mel, method="pinv", n_iters=100, lengths=None):
        """Addition, not in the reference: log-mel [B, n_mel, T] (or [n_mel, T]) -> linear magnitudes [B, n_fft/2+1, T]
        (or [n_fft/2+1, T]) = relu(pinv(mel_basis) @ spectral_de_normalize(mel)), the product on ft_gemm in fp32 with the
        ReLU epilogue, one batched call.  Frames after an utterance's end that hold zeros decode as magnitude 1, not
        silence: a batch of different lengths goes to mel_to_magnitude_ragged.
        method="nnls": the ReLU clips what the pseudo-inverse made negative, and the result no longer maps back onto the mel;
        one more launch (ft_mel_nnls, csrc/vocode.hip) takes it as the start of n_iters multiplicative updates of
        min ||mel_basis m - exp(mel)||^2 over m >= 0, the mel inversion of the common Python audio library (n_fft 256 .. 4096, at
        most 128 bands that overlap at most pairwise).  Bins that no band covers stay 0.
        lengths (host integers, one per utterance): mel_to_magnitude_ragged's result with this method -- zeros behind every
        utterance, with method="nnls" written by ft_mel_nnls itself, which does not read the frames behind an utterance's end;
        mel_to_magnitude_ragged keeps its signature and is this call at method="pinv"."""
        _check_inversion(method, n_iters)
        if lengths is not None:
            lens = self._check_ragged_mel(mel, lengths, "mel_to_magnitude")
            return self._mel_to_magnitude(mel, method, n_iters, lens, "mel_to_magnitude")
        L.require_cuda(mel)
        if mel.dim() not in (2, 3) or mel.shape[-2] != self.n_mel_channels:
            raise ValueError("mel_to_magnitude needs [B, %d, T] or [%d, T], got %s"
                             % (self.n_mel_channels, self.n_mel_channels, tuple(mel.shape)))
        return self._mel_to_magnitude(mel, method, n_iters, None, "mel_to_magnitude")

    def mel_to_audio(self, mel, n_iters=30, momentum=0.0, inversion="pinv", inversion_iters=100, lengths=None, angles=None,
                     phase_init="random"):
        """Addition, not in the reference: log-mel [B, n_mel, T] (a dense batch, e.g. Flowtron.infer's output) or [n_mel, T]
        -> waveform [B, hop * (T - 1)] (or [hop * (T - 1)]) = griffin_lim(mel_to_magnitude(mel, inversion, inversion_iters),
        self.stft_fn, n_iters, momentum).  Every utterance of a batch must fill all T frames (zeros decode as magnitude 1, not
        silence): a batch of different lengths, such as Flowtron.infer(..., return_lengths=True) returns, goes to
        mel_to_audio_ragged, or here with lengths= (host integers) and optionally angles= (mel_to_audio_ragged's starting
        phase): mel_to_audio_ragged's pass with these options, utterance b still bit for bit the same call on it alone.
        mel_to_audio_ragged keeps its signature and is this call at the defaults.
        phase_init="spsi": Griffin-Lim starts from spsi_phase of the inverted magnitudes instead of the random draw (griffin_lim's
        phase_init; refused together with angles=); with n_iters=0 the whole vocode is three launches after the pseudo-inverse:
        NNLS, ft_spsi_phase and one inverse STFT."""
        _check_inversion(inversion, inversion_iters)
        momentum = _check_momentum(momentum)
        phase_init = _check_phase_init(phase_init, angles)
        if lengths is not None:
            return self._mel_to_audio_ragged(mel, lengths, n_iters, angles, momentum, inversion, inversion_iters, phase_init)
        if angles is not None:
            raise ValueError("mel_to_audio takes starting angles only with lengths (the dense call draws them as the reference does)")
        mag = self.mel_to_magnitude(mel, inversion, inversion_iters)
        y = griffin_lim(mag if mag.dim() == 3 else mag[None], self.stft_fn, n_iters, momentum, phase_init=phase_init)
        return y if mel.dim() == 3 else y[0]

    def _check_ragged_mel(self, mel, lengths, what):
        L.require_cuda(mel)
        if mel.dim() != 3 or mel.shape[1] != self.n_mel_channels:
            raise ValueError("%s needs [B, %d, T], got %s" % (what, self.n_mel_channels, tuple(mel.shape)))
        B, _, T = mel.shape
        return _host_lengths(lengths, B, 1, T, "lengths", "1 ..= T = %d" % T)

    def mel_to_magnitude_ragged(self, mel, lengths):
        """mel_to_magnitude for a batch of different lengths: log-mel [B, n_mel, T], utterance b holds lengths[b] frames (host
        integers) -> [B, n_fft/2+1, T] with mel_to_magnitude's values inside each utterance and zero behind it.  The NNLS
        inversion of a ragged batch is mel_to_magnitude(mel, method="nnls", lengths=lengths)."""
        lens = self._check_ragged_mel(mel, lengths, "mel_to_magnitude_ragged")
        return self._mel_to_magnitude(mel, "pinv", 100, lens, "mel_to_magnitude_ragged")

    def mel_to_audio_ragged(self, mel, lengths, n_iters=30, angles=None):
        """mel_to_audio for a batch of different lengths in one Griffin-Lim pass: log-mel [B, n_mel, T] and the frames each
        utterance holds (host integers: Flowtron.infer(..., in_lens=, out_lens=, return_lengths=True) returns both) -> waveform
        [B, hop * (T - 1)] = griffin_lim_ragged(mel_to_magnitude(mel), lengths, self.stft_fn, n_iters, angles): utterance b
        occupies [: hop * (lengths[b] - 1)], zeros behind.  The frames behind an utterance's end are never read by the loop.
        Momentum and the NNLS inversion for a ragged batch: mel_to_audio(mel, ..., lengths=lengths, angles=angles)."""
        return self._mel_to_audio_ragged(mel, lengths, n_iters, angles, 0.0, "pinv", 100)

    def _mel_to_audio_ragged(self, mel, lengths, n_iters, angles, momentum, inversion, inversion_iters, phase_init="random"):
        L.require_cuda(mel)
        self.stft_fn._require_device_path("TacotronSTFT.mel_to_audio_ragged")
        lens = self._check_ragged_mel(mel, lengths, "mel_to_audio_ragged")
        _check_reflect(lens, self.stft_fn, "mel_to_audio_ragged", "lengths")
        if inversion == "pinv":
            mag = self.mel_to_magnitude(mel)
        else:
            mag = self._mel_to_magnitude(mel, inversion, inversion_iters, lens, "mel_to_audio_ragged")
        return _griffin_lim_ragged(mag, lens, self.stft_fn, n_iters, angles, momentum, phase_init)
