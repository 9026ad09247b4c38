"""Endpoints and loudness on the device: trim leading and trailing silence, measure ITU-R BS.1770-4 integrated loudness, bring a
corpus to one level (additive: the reference only divides by the peak at the end of inference.py; csrc/level.hip).

    start, end = level.active_bounds(audio, n_samples, top_db=60.0)             # librosa.effects.trim's rule, per utterance
    trimmed, n_out = level.trim(audio, n_samples, top_db=60.0)                  # [start, end) to the front, zeros behind
    lufs, power = level.loudness(audio, n_samples, 22050)                       # K-weighting, 400 ms blocks, both gates
    out, gain = level.normalize(audio, n_samples, 22050, target_lufs=-23.0)
    out, n_out, info = level.prepare(audio, n_samples, 22050)                   # bounds, loudness of the span, gain, one gather
    mel = stft.mel_spectrogram_ragged(out, n_out)                               # n_out is an int32 tensor on the device

audio is [N] or [B, N] fp32 on the device, a zero-padded batch; n_samples a host sequence of B integers in 1 ..= N, or an int32
tensor on the device (the kernels clamp it to 1 ..= N), which is what lets the steps chain: no function here synchronises with
the host.  Samples behind an utterance's end are never read, and every utterance gives the same bits alone as inside any batch.
include/flowtron_hip.h states the arithmetic; tests/level_ref.py replays it bit for bit.  The endpoint rule is unpinned against
librosa and the loudness against any loudness library (neither was available): the loudness is pinned to the standard's
coefficient table and its 997 Hz level, the filter to scipy.signal.lfilter in float64."""
from __future__ import annotations

import collections
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import _lib as L
from .model import lengths_arg

CHUNK = 256                # FT_LEVEL_CHUNK: the samples a lane filters; a 100 ms step must hold at least as many
MAX_STEPS = 4096           # FT_LEVEL_MAX_STEPS: 100 ms steps of the longest utterance (409.6 s)
MAX_FRAME = 4096           # FT_LEVEL_MAX_FRAME
MAX_BATCH = 65535
ABSOLUTE_GATE_LUFS = -70.0
LUFS_OFFSET = -0.691

Loudness = collections.namedtuple("Loudness", "lufs power step_sums peak")
Bounds = collections.namedtuple("Bounds", "power peak start end")
PrepareInfo = collections.namedtuple("PrepareInfo", "start end lufs gain peak")


# ---- host tables (float64; the replay in tests/level_ref.py uses these very functions) -------------------------------------------

def k_weighting(sampling_rate):
    """-> (shelf b [3], shelf a [3], high-pass b [3], high-pass a [3]): the K-weighting biquads of BS.1770-4 for this rate, by
    the bilinear form that reproduces the standard's 48 kHz table (re-derived per rate, not resampled)."""
    fs = float(sampling_rate)
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Q = 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    sb = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0)
    sa = (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    ha = (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    return sb, sa, (1.0, -2.0, 1.0), ha


def filter_coefficients(sampling_rate):
    """-> the seven doubles ft_level_loudness takes: shelf b0 b1 b2 a1 a2, high-pass a1 a2"""
    sb, sa, _, ha = k_weighting(sampling_rate)
    return (sb[0], sb[1], sb[2], sa[1], sa[2], ha[1], ha[2])


def carry_matrix(coef, chunk=CHUNK):
    """-> M [4][4] (lists of Python floats): column j is the state (v1, v2, y1, y2) after `chunk` steps of the cascade with no
    input from the j-th unit state, every operation a float64 operation in the kernels' order."""
    a1, a2, h1, h2 = coef[3], coef[4], coef[5], coef[6]
    M = [[0.0] * 4 for _ in range(4)]
    for j in range(4):
        v1, v2, y1, y2 = [1.0 if i == j else 0.0 for i in range(4)]
        for _ in range(chunk):
            v = (0.0 - a1 * v1) - a2 * v2
            y = (((v - 2.0 * v1) + v2) - h1 * y1) - h2 * y2
            v2, v1, y2, y1 = v1, v, y1, y
        for r, val in enumerate((v1, v2, y1, y2)):
            M[r][j] = val
    return M


def absolute_gate_power():
    """the block power at -70 LUFS"""
    return 10.0 ** ((ABSOLUTE_GATE_LUFS - LUFS_OFFSET) / 10.0)


def threshold_power(top_db):
    """10^(-top_db / 10), formed in float64 and rounded once to fp32"""
    return float(np.float32(10.0 ** (-float(top_db) / 10.0)))


def block_step(sampling_rate):
    """the samples of a 100 ms step; a block is four (at 11,025 Hz a block is 4408 samples, not 4410)"""
    return int(sampling_rate) // 10


# ---- argument checks ----------------------------------------------------------------------------------------------------------------

def _int_arg(v, name, lo):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < lo:
        raise ValueError("%s must be an integer >= %d, got %r" % (name, lo, v))
    return int(v)


def _pos_arg(v, name):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v <= 0:
        raise ValueError("%s must be a positive finite number, got %r" % (name, v))
    return float(v)


def _real_arg(v, name):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError("%s must be a finite number, got %r" % (name, v))
    return float(v)


def _audio_arg(audio, who):
    if not torch.is_tensor(audio) or audio.dim() not in (1, 2):
        raise ValueError("audio must be a [N] or [B, N] tensor, got %s" % ((tuple(audio.shape) if torch.is_tensor(audio) else type(audio).__name__),))
    if min(audio.shape) < 1:
        raise ValueError("audio must hold at least one utterance and one sample, got shape %s" % (tuple(audio.shape),))
    if audio.dtype != torch.float32:
        raise ValueError("audio must be float32, got %s" % audio.dtype)
    single = audio.dim() == 1
    a2 = audio[None] if single else audio
    if a2.shape[0] > MAX_BATCH:
        raise NotImplementedError("%s holds at most %d utterances a call, got %d" % (who, MAX_BATCH, a2.shape[0]))
    return a2.detach(), single


def _device_i32(v, name, B):
    """a [B] int32 tensor on the device is taken as it is: reading it would synchronise"""
    if v.dim() != 1 or v.shape[0] != B:
        raise ValueError("%s must be one-dimensional with %d entries, got shape %s" % (name, B, tuple(v.shape)))
    return v.contiguous()


def _lengths(n_samples, a2):
    """-> (int32 [B] on the device, host list or None)"""
    B, N = a2.shape
    if torch.is_tensor(n_samples) and n_samples.is_cuda and n_samples.dtype == torch.int32:
        return _device_i32(n_samples, "n_samples", B), None
    ln = lengths_arg(n_samples, "n_samples", B, N)
    L.require_cuda(a2)
    ln = ln if ln is not None else [N] * B
    return torch.tensor(ln, dtype=torch.int32, device=a2.device), ln


def _span_arg(v, name, B):
    if v is None:
        return None
    if not torch.is_tensor(v) or v.dtype != torch.int32 or not v.is_cuda:
        raise ValueError("%s must be an int32 tensor on the device (as active_bounds returns it) or None, got %s"
                         % (name, (v.dtype, str(v.device)) if torch.is_tensor(v) else type(v).__name__))
    return _device_i32(v.reshape(-1) if v.dim() == 0 else v, name, B)


def _frame_args(top_db, frame_length, hop_length, ref, pad):
    thr = threshold_power(_pos_arg(top_db, "top_db"))
    F = _int_arg(frame_length, "frame_length", 2)
    hop = _int_arg(hop_length, "hop_length", 1)
    if F % 2:
        raise ValueError("frame_length must be even, got %d" % F)
    if hop > F:
        raise ValueError("hop_length must not exceed frame_length, got %d and %d" % (hop, F))
    if F > MAX_FRAME:
        raise NotImplementedError("a frame holds at most %d samples (MAX_FRAME), got frame_length %d" % (MAX_FRAME, F))
    if isinstance(ref, str):
        if ref != "max":
            raise ValueError("ref must be 'max' or a positive power, got %r" % (ref,))
        ref_power = 0.0
    else:
        ref_power = float(np.float32(_pos_arg(ref, "ref")))
        if not (ref_power > 0.0 and math.isfinite(ref_power)):
            raise ValueError("ref must be a positive power that fp32 holds, got %r" % (ref,))
    return thr, F, hop, ref_power, _int_arg(pad, "pad", 0)


def _rate_arg(sampling_rate, N):
    if isinstance(sampling_rate, bool) or not isinstance(sampling_rate, numbers.Integral) or sampling_rate < 1:
        raise ValueError("sampling_rate must be a positive integer, got %r" % (sampling_rate,))
    sr = int(sampling_rate)
    step = block_step(sr)
    if step < CHUNK:
        raise NotImplementedError("loudness holds sampling rates of at least %d Hz (a 100 ms step of at least CHUNK = %d samples), got %d"
                                  % (10 * CHUNK, CHUNK, sr))
    if N // step > MAX_STEPS:
        raise NotImplementedError("loudness holds at most %d steps of 100 ms an utterance (MAX_STEPS, %.1f s), got %d samples at %d Hz"
                                  % (MAX_STEPS, MAX_STEPS / 10.0, N, sr))
    return sr, step


def _gain_args(target_lufs, peak_ceiling, max_gain_db):
    target = None if target_lufs is None else _real_arg(target_lufs, "target_lufs")
    ceiling = None if peak_ceiling is None else _pos_arg(peak_ceiling, "peak_ceiling")
    return target, ceiling, _real_arg(max_gain_db, "max_gain_db")


# ---- launches -----------------------------------------------------------------------------------------------------------------------

def _bounds(a2, n32, thr, F, hop, ref_power, pad):
    B, N = a2.shape
    T = N // hop + 1
    dev = a2.device
    power = torch.empty(B, T, dtype=torch.float32, device=dev)
    frame_peak = torch.empty(B, T, dtype=torch.float32, device=dev)
    peak = torch.empty(B, dtype=torch.float32, device=dev)
    start = torch.empty(B, dtype=torch.int32, device=dev)
    end = torch.empty(B, dtype=torch.int32, device=dev)
    L.check(L.lib().ft_level_bounds(L.ptr(a2), *a2.stride(), L.ptr(n32), L.ptr(power), L.ptr(frame_peak), L.ptr(peak), L.ptr(start),
                                    L.ptr(end), B, N, F, hop, thr, ref_power, pad, L.stream()), "ft_level_bounds")
    return Bounds(power, peak, start, end)


_HOST_TABLES = {}          # sampling rate -> (coef, carry) as ctypes arrays, and the gate


def _filter_tables(sr):
    if sr not in _HOST_TABLES:
        coef = filter_coefficients(sr)
        M = carry_matrix(coef)
        _HOST_TABLES[sr] = ((C.c_double * 7)(*coef), (C.c_double * 16)(*[M[r][j] for r in range(4) for j in range(4)]))
    return _HOST_TABLES[sr]


def _loudness(a2, n32, sr, step, start, end):
    B, N = a2.shape
    dev = a2.device
    S = max(N // step, 1)
    coef, carry = _filter_tables(sr)
    step_sums = torch.empty(B, S, dtype=torch.float64, device=dev)
    power = torch.empty(B, dtype=torch.float64, device=dev)
    peak = torch.empty(B, dtype=torch.float32, device=dev)
    nbytes = L.lib().ft_level_loudness_workspace_bytes(B, N)
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    L.check(L.lib().ft_level_loudness(L.ptr(a2), *a2.stride(), L.ptr(n32), L.ptr(start), L.ptr(end), coef, carry, absolute_gate_power(),
                                      L.ptr(step_sums), L.ptr(power), L.ptr(peak), L.ptr(work), work.numel() * 8, B, N, step,
                                      L.stream()), "ft_level_loudness")
    lufs = LUFS_OFFSET + 10.0 * torch.log10(power)
    return Loudness(lufs, power, step_sums, peak)


def _gather(a2, n32, start, end, gain):
    B, N = a2.shape
    out = torch.empty(B, N, dtype=torch.float32, device=a2.device)
    n_out = torch.empty(B, dtype=torch.int32, device=a2.device)
    L.check(L.lib().ft_level_gather(L.ptr(a2), *a2.stride(), L.ptr(n32), L.ptr(start), L.ptr(end), L.ptr(gain), L.ptr(out),
                                    L.ptr(n_out), B, N, L.stream()), "ft_level_gather")
    return out, n_out


def _gain_arg(gain, B, dev):
    if gain is None:
        return None
    if not torch.is_tensor(gain) or gain.dtype != torch.float32 or gain.dim() > 1 or gain.numel() != B:
        raise ValueError("gain must be a float32 tensor of %d entries, got %s" % (B, (tuple(gain.shape), gain.dtype) if torch.is_tensor(gain) else type(gain).__name__))
    L.require_cuda(gain)
    return gain.detach().reshape(B).contiguous()


def gain_for(lufs, peak, target_lufs=-23.0, peak_ceiling=0.99, max_gain_db=30.0):
    """lufs [B] float64, peak [B] fp32 -> the gain [B] fp32, float64 torch arithmetic on the tensors' device rounded once:
    10^((target_lufs - lufs) / 20), 1 where lufs is NaN or infinite, at most 10^(max_gain_db / 20), then lowered to
    peak_ceiling / peak where gain * peak would exceed peak_ceiling (None: no ceiling).  target_lufs=None: peak_ceiling / peak
    (the reference's peak normalisation; 1 for a peak of 0), at most 10^(max_gain_db / 20)."""
    target, ceiling, max_db = _gain_args(target_lufs, peak_ceiling, max_gain_db)
    one = torch.ones_like(lufs)
    cap = 10.0 ** (max_db / 20.0)
    pk = peak.to(torch.float64)
    if target is None:
        g = one if ceiling is None else torch.where(pk > 0, ceiling / pk, one)
        g = torch.clamp(g, max=cap)
    else:
        g = torch.pow(10.0, (target - lufs) / 20.0)
        g = torch.where(torch.isfinite(lufs), g, one)
        g = torch.clamp(g, max=cap)
        if ceiling is not None:
            g = torch.where(g * pk > ceiling, ceiling / pk, g)
    return g.to(torch.float32)


# ---- the public calls ---------------------------------------------------------------------------------------------------------------

def frame_power(audio, n_samples=None, frame_length=2048, hop_length=512):
    """The energy contour: [B, T] fp32 ([T] for [N]), T = N // hop_length + 1, the mean square of the frame_length samples
    centred on sample t * hop_length (samples outside the utterance count as 0), summed in float64 and rounded once; 0 behind
    an utterance's n // hop_length + 1 frames.  With pitch.f0's hop and window these are pitch.f0's frames."""
    a2, single = _audio_arg(audio, "frame_power")
    thr, F, hop, ref_power, pad = _frame_args(60.0, frame_length, hop_length, "max", 0)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    power = _bounds(a2, n32, thr, F, hop, ref_power, pad).power
    return power[0] if single else power


def active_bounds(audio, n_samples=None, top_db=60.0, frame_length=2048, hop_length=512, ref="max", pad=0, return_all=False):
    """Where an utterance's sound starts and ends, by librosa.effects.trim's rule (unpinned against librosa): frame t (t = 0 ..
    n // hop_length) is centred on sample t * hop_length, its power is the mean square, and it is active iff
    power > 10^(-top_db / 10) * ref_power, ref_power the utterance's largest frame power (ref="max") or a given power (ref=1.0:
    full scale).  -> (start, end), int32 [B] on the device (0-dim for [N]): start = first_active * hop_length,
    end = min(n, (last_active + 1) * hop_length), both widened by pad samples inside [0, n].  An utterance without an active
    frame (digital silence, nothing above an absolute ref), or whose one active frame is centred on its end, keeps (0, n):
    nothing downstream takes an empty utterance.  The comparison is made in the power domain in float64; no logarithm is
    taken.  return_all: the Bounds tuple (power [B, T], peak [B] = max |x| over [0, n), start, end).
    NotImplementedError for frame_length > 4096 or more than 65,535 utterances; two launches."""
    a2, single = _audio_arg(audio, "active_bounds")
    thr, F, hop, ref_power, pad = _frame_args(top_db, frame_length, hop_length, ref, pad)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    r = _bounds(a2, n32, thr, F, hop, ref_power, pad)
    if single:
        r = Bounds(*[x[0] for x in r])
    return r if return_all else (r.start, r.end)


def trim(audio, n_samples=None, top_db=60.0, frame_length=2048, hop_length=512, ref="max", pad=0, gain=None):
    """active_bounds, then one gather: -> (trimmed [B, N] with [start, end) of every utterance at the front and zeros behind,
    n_out int32 [B] on the device = end - start).  gain [B] fp32 on the device multiplies every sample, one fp32 rounding.
    Three launches, nothing on the host between them."""
    a2, single = _audio_arg(audio, "trim")
    thr, F, hop, ref_power, pad = _frame_args(top_db, frame_length, hop_length, ref, pad)
    g = _gain_arg(gain, a2.shape[0], a2.device)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    r = _bounds(a2, n32, thr, F, hop, ref_power, pad)
    out, n_out = _gather(a2, n32, r.start, r.end, g)
    return (out[0], n_out[0]) if single else (out, n_out)


def loudness(audio, n_samples=None, sampling_rate=22050, start=None, end=None, return_all=False):
    """ITU-R BS.1770-4 integrated loudness, one channel: K-weighting (coefficients re-derived for sampling_rate), blocks of four
    steps of sampling_rate // 10 samples with 75 % overlap, the absolute gate at -70 LUFS and the relative gate 10 LU below the
    mean of what passed it -> (lufs [B] float64 = -0.691 + 10 log10(power), formed by torch; power [B] float64, the gated mean
    square, which a float64 replay equals bit for bit).  An utterance shorter than a block gives NaN, one with no block above
    the absolute gate power 0 and lufs -inf.  start / end: int32 tensors on the device (as active_bounds returns them): the
    span [start, end) is measured in place, the filter starting from a zero state at start, exactly as if the trimmed
    utterance were measured alone.  return_all: the Loudness tuple (lufs, power, step_sums [B, max(N // step, 1)] float64, peak [B] =
    max |x| over the span).  Four launches.  NotImplementedError below 2560 Hz, for more than 4096 steps (409.6 s) in N, or
    more than 65,535 utterances."""
    a2, single = _audio_arg(audio, "loudness")
    sr, step = _rate_arg(sampling_rate, a2.shape[1])
    B = a2.shape[0]
    s32, e32 = _span_arg(start, "start", B), _span_arg(end, "end", B)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    r = _loudness(a2, n32, sr, step, s32, e32)
    if single:
        r = Loudness(*[x[0] for x in r])
    return r if return_all else (r.lufs, r.power)


def normalize(audio, n_samples=None, sampling_rate=22050, target_lufs=-23.0, peak_ceiling=0.99, max_gain_db=30.0):
    """Bring every utterance to target_lufs: -> (out [B, N] = fp32(gain * audio) with zeros behind each utterance, gain [B] fp32).
    The gain is gain_for's: capped at max_gain_db, lowered to peak_ceiling / peak where it would clip, 1 where the loudness is
    undefined (shorter than 400 ms) or -inf (silence).  target_lufs=None with peak_ceiling= is the reference's peak
    normalisation alone."""
    a2, single = _audio_arg(audio, "normalize")
    target, ceiling, max_db = _gain_args(target_lufs, peak_ceiling, max_gain_db)
    if target is not None:
        sr, step = _rate_arg(sampling_rate, a2.shape[1])
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    if target is None:
        r = _bounds(a2, n32, *_frame_args(60.0, 2048, 512, "max", 0))
        lufs, peak = torch.full_like(r.peak, float("nan"), dtype=torch.float64), r.peak
    else:
        r = _loudness(a2, n32, sr, step, None, None)
        lufs, peak = r.lufs, r.peak
    gain = gain_for(lufs, peak, target, ceiling, max_db)
    out, _ = _gather(a2, n32, None, None, gain)
    return (out[0], gain[0]) if single else (out, gain)


def prepare(audio, n_samples=None, sampling_rate=22050, top_db=60.0, target_lufs=-23.0, peak_ceiling=0.99, max_gain_db=30.0,
            frame_length=2048, hop_length=512, ref="max", pad=0):
    """Corpus preparation in one pass over a batch already at its final rate: active_bounds, the loudness of the span
    [start, end) in place, gain_for, one gather with the gain -> (out [B, N], n_out int32 [B] on the device,
    PrepareInfo(start, end, lufs, gain, peak)): lufs is the trimmed utterance's loudness before the gain, peak its max |x|
    before the gain; all on the device.  Equal, bit for bit, to trim, loudness of the trimmed batch, and normalize's gain.
    Three entry calls (ft_level_bounds, ft_level_loudness, ft_level_gather: seven launches) and a few torch elementwise ones
    for the gain; nothing synchronises.  n_out goes straight into TacotronSTFT.mel_spectrogram_ragged(out, n_out)."""
    a2, single = _audio_arg(audio, "prepare")
    thr, F, hop, ref_power, pad = _frame_args(top_db, frame_length, hop_length, ref, pad)
    target, ceiling, max_db = _gain_args(target_lufs, peak_ceiling, max_gain_db)
    sr, step = _rate_arg(sampling_rate, a2.shape[1])
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    bd = _bounds(a2, n32, thr, F, hop, ref_power, pad)
    ld = _loudness(a2, n32, sr, step, bd.start, bd.end)
    gain = gain_for(ld.lufs, ld.peak, target, ceiling, max_db)
    out, n_out = _gather(a2, n32, bd.start, bd.end, gain)
    info = PrepareInfo(bd.start, bd.end, ld.lufs, gain, ld.peak)
    if single:
        return out[0], n_out[0], PrepareInfo(*[x[0] for x in info])
    return out, n_out, info
