"""Mel-cepstral distortion along a dynamic-time-warping path (MCD-DTW): how far a synthesized mel is from a reference mel of
another length, in dB (additive: the reference has no metric of its own; csrc/dtw.hip).

    mel, _, n_frames = model.infer(residual, speaker_ids, text, return_lengths=True)  # [B, M, N] log-mel, frames per utterance
    mcd = mel_cepstral_distortion(mel, n_frames, recorded_mel, out_lens)              # [B] dB, one launch for the warp

    cep = mel_cepstra(mel, lens, n_coeffs=13)                                         # [B, T, K] cepstra 1 .. K (no c0)
    cost, path, path_len = dtw(cep_a, cep_b, a_lens, b_lens)                          # the warp itself, on any features
    rmse_cents, vuv_error, n_voiced = f0_distortion(f0_a, f0_b, path, path_len)       # pitch error along a path (pitch.f0)
    mcd = envelope_cepstral_distortion(audio_a, n_a, f0_a, audio_b, n_b, f0_b)        # [B] dB on mel-cepstra of the F0-adaptive
                                                                                      # envelope: the one to use where the pitch differs

Everything runs on the device and refuses tensors on the host; lengths are lists or integer tensors, on the host or the
device (read to the host once, as Flowtron.infer reads them)."""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from . import _lib as L
from . import ops
from .model import lengths_arg

MAX_FRAMES = 1024          # ft_dtw_ragged: one thread per frame of the second sequence, the first one's frames in LDS
MAX_COEFFS = 32
MAX_MELS = 128
MAX_LAG = 1022             # ft_f0_yin_ragged (pitch.f0): the longest lag tau_max = ceil(sampling_rate / fmin)

MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)

_DCT = {}


def dct_table(n_mels, n_coeffs):
    """rows 1 .. n_coeffs of the orthonormal DCT-II over n_mels points, [K, M]: sqrt(2 / M) cos(pi k (m + 0.5) / M), formed in
    float64 and rounded to float32 once (host tensor)."""
    k = np.arange(1, n_coeffs + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return torch.from_numpy((np.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (m + 0.5) / n_mels)).astype(np.float32))


def _mel_arg(mel, name):
    if not torch.is_tensor(mel) or mel.dim() != 3:
        raise ValueError("%s must be a [B, M, T] tensor, got %s" % (name, tuple(mel.shape) if torch.is_tensor(mel) else type(mel).__name__))
    if min(mel.shape) < 1:
        raise ValueError("%s must hold at least one utterance, channel and frame, got shape %s" % (name, tuple(mel.shape)))
    if mel.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, mel.dtype))
    return mel.shape


def _coeffs_arg(n_coeffs, n_mels):
    if isinstance(n_coeffs, bool) or not isinstance(n_coeffs, numbers.Integral) or not 1 <= n_coeffs <= MAX_COEFFS:
        raise ValueError("n_coeffs must be an integer in 1 ..= %d, got %r" % (MAX_COEFFS, n_coeffs))
    if n_coeffs >= n_mels:
        raise ValueError("n_coeffs must be below the %d mel channels, got %d" % (n_mels, n_coeffs))
    if n_mels > MAX_MELS:
        raise ValueError("mel_cepstra holds at most %d mel channels, got %d" % (MAX_MELS, n_mels))
    return int(n_coeffs)


def _cepstra(mel, lens, K):
    """validated arguments -> [B, T, K] (lens: list of ints or None)"""
    B, M, T = mel.shape
    key = (M, K, mel.device)
    if key not in _DCT:
        _DCT[key] = dct_table(M, K).to(mel.device)
    l32 = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=mel.device)
    return ops.mel_cepstra(mel.detach(), l32, _DCT[key])


def mel_cepstra(mel, lens=None, n_coeffs=13):
    """Truncated cepstra of log-mel frames: mel [B, M, T] (fp32 on the device, any view: read in place through its strides)
    -> [B, T, K] fp32, cep[b, t, k-1] = sum_m mel[b, m, t] sqrt(2 / M) cos(pi k (m + 0.5) / M) for k = 1 .. K = n_coeffs (the
    orthonormal DCT-II without c0, the energy term), summed over ascending m in fp32.  lens: frames per utterance, 1 ..= T
    (None: T); rows at or behind lens[b] are 0 and their frames are never read.  1 <= n_coeffs <= 32, n_coeffs < M <= 128."""
    B, M, T = _mel_arg(mel, "mel")
    K = _coeffs_arg(n_coeffs, M)
    ln = lengths_arg(lens, "lens", B, T)
    L.require_cuda(mel)
    return _cepstra(mel, ln, K)


def _features_arg(x, y):
    for t, name in ((x, "x"), (y, "y")):
        if not torch.is_tensor(t) or t.dim() != 3:
            raise ValueError("%s must be a [B, T, K] tensor, got %s" % (name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        if min(t.shape) < 1:
            raise ValueError("%s must hold at least one pair, frame and feature, got shape %s" % (name, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (name, t.dtype))
    if x.shape[0] != y.shape[0]:
        raise ValueError("x holds %d sequences and y %d: one pair per utterance" % (x.shape[0], y.shape[0]))
    if x.shape[2] != y.shape[2]:
        raise ValueError("x has %d features per frame and y %d" % (x.shape[2], y.shape[2]))
    if x.shape[2] > MAX_COEFFS:
        raise ValueError("dtw holds at most %d features per frame, got %d" % (MAX_COEFFS, x.shape[2]))


def _pair_lengths(xl, yl, B, Ta, Tb, names, diagonal, what):
    """-> (list, list), each 1 ..= its T (None: T everywhere); the refusals that depend on the lengths"""
    xl = lengths_arg(xl, names[0], B, Ta) or [Ta] * B
    yl = lengths_arg(yl, names[1], B, Tb) or [Tb] * B
    if diagonal:
        bad = [b for b in range(B) if xl[b] != yl[b]]
        if bad:
            raise ValueError("%s compares frame by frame and needs equal lengths: pair %d has %d and %d frames"
                             % (what, bad[0], xl[bad[0]], yl[bad[0]]))
    if max(Ta, Tb) > MAX_FRAMES:
        raise NotImplementedError("dtw holds at most %d frames per side (MAX_FRAMES), got %d and %d" % (MAX_FRAMES, Ta, Tb))
    return xl, yl


def _dtw(x, y, xl, yl, diagonal):
    x32 = torch.tensor(xl, dtype=torch.int32, device=x.device)
    y32 = torch.tensor(yl, dtype=torch.int32, device=x.device)
    return ops.dtw_ragged(x.detach(), y.detach(), x32, y32, diagonal)


def dtw(x, y, x_lens=None, y_lens=None, diagonal=False):
    """Dynamic time warping of one pair of feature sequences per utterance, the whole batch in one launch: x [B, Ta, K] and
    y [B, Tb, K] (fp32 on the device, any strides), A = x_lens[b] and N = y_lens[b] frames (None: all).  The distance of two
    frames is the Euclidean one; a path runs from (0, 0) to (A - 1, N - 1) in steps (1, 1), (1, 0) or (0, 1); among the
    cheapest paths the one whose LAST step prefers (1, 1) over (1, 0) over (0, 1), and so on backwards (x and y are not
    interchangeable on ties).  All arithmetic is fp32, one rounding per operation, so a float32 replay gives the same bits.
    -> (cost [B] fp32: the summed distance along the path; path [B, Ta + Tb - 1, 2] int32: its cells (i, j) in ascending
    order, -1 behind path_len; path_len [B] int32).  diagonal: the cells (i, i) only -- ValueError unless every pair has
    equal lengths.  Features behind the lengths are never read.  NotImplementedError above MAX_FRAMES = 1024 frames a side."""
    _features_arg(x, y)
    B, Ta, _ = x.shape
    xl, yl = _pair_lengths(x_lens, y_lens, B, Ta, y.shape[1], ("x_lens", "y_lens"), diagonal, "diagonal=True")
    L.require_cuda(x, y)
    return _dtw(x, y, xl, yl, diagonal)


def mel_cepstral_distortion(mel_a, a_lens, mel_b, b_lens, n_coeffs=13, align=True, return_path=False):
    """Mel-cepstral distortion in dB between two batches of log-mel spectrograms, pair by pair: mel_a [B, M, Ta] and mel_b
    [B, M, Tb] (fp32 on the device, any views), a_lens / b_lens their frames (None: all).
        mcd[b] = (10 / ln 10) sqrt(2) * mean over the path's cells (i, j) of || cep_a[i] - cep_b[j] ||
    with cepstra 1 .. n_coeffs (no c0) and, for align=True, the dynamic-time-warping path of dtw() -- so utterances of different
    lengths compare (MCD-DTW); align=False compares frame i with frame i and needs equal lengths (a teacher-forced or
    infer_aligned reconstruction).  The mean is cost / path_len in float64 on the device, rounded to fp32 once.
    This is the distortion of cepstra of the PROJECT'S OWN log-mel (natural logarithm of the clamped mel magnitudes,
    audio_processing.dynamic_range_compression), the quantity the model is trained on; it is not computed on WORLD / SPTK
    mel-cepstra and its numbers do not compare with papers that use those.
    -> mcd [B] fp32, and with return_path also (path [B, Ta + Tb - 1, 2] int32, path_len [B] int32)."""
    B, M, Ta = _mel_arg(mel_a, "mel_a")
    Bb, Mb, Tb = _mel_arg(mel_b, "mel_b")
    if Bb != B:
        raise ValueError("mel_a holds %d utterances and mel_b %d: one pair per utterance" % (B, Bb))
    if Mb != M:
        raise ValueError("mel_a has %d mel channels and mel_b %d" % (M, Mb))
    K = _coeffs_arg(n_coeffs, M)
    al, bl = _pair_lengths(a_lens, b_lens, B, Ta, Tb, ("a_lens", "b_lens"), not align, "align=False")
    L.require_cuda(mel_a, mel_b)
    cost, path, path_len = _dtw(_cepstra(mel_a, al, K), _cepstra(mel_b, bl, K), al, bl, not align)
    mcd = (MCD_SCALE * cost.double() / path_len.double()).float()
    return (mcd, path, path_len) if return_path else mcd


def envelope_cepstral_distortion(audio_a, n_a, f0_a, audio_b, n_b, f0_b, sampling_rate=22050, hop_length=256, order=24, alpha=None,
                                 align=True, return_path=False):
    """Mel-cepstral distortion in dB as the papers compute it, between two batches of WAVEFORMS, pair by pair: mel-cepstra
    1 .. order (no c0) of the F0-adaptive spectral envelope (envelope.mel_cepstra: CheapTrick, SPTK's frequency transform with
    all-pass constant alpha, None = the customary value for the rate) of audio_a [B, Na] and audio_b [B, Nb] (fp32 on the
    device, zero-padded), n_a / n_b their samples (lists or integer tensors, read to the host once; None: all), f0_a / f0_b
    their pitch tracks in Hz at this hop (pitch.f0 or pitch.f0_track).  The envelope does not resolve the harmonics, so the
    figure does not move with F0 the way mel_cepstral_distortion's does: use this one whenever the two sides differ in pitch.
        mcd[b] = (10 / ln 10) sqrt(2) * mean over the path's cells (i, j) of || mc_a[i, 1:] - mc_b[j, 1:] ||
    along the path of dtw() over n // hop_length + 1 frames a side (align=False: frame i with frame i, equal frame counts),
    formed as mel_cepstral_distortion forms it; the coefficients go through dtw() as strided views of the kernel's output.
    The frames are the F0 track's, at the STFT hop, not the 5 ms of most papers; NOT pinned against pyworld / pysptk.
    -> mcd [B] fp32, and with return_path also (path [B, Ta + Tb - 1, 2] int32, path_len [B] int32), which f0_distortion takes."""
    from . import envelope
    for a, name in ((audio_a, "audio_a"), (audio_b, "audio_b")):
        if not torch.is_tensor(a) or a.dim() != 2:
            raise ValueError("%s must be a [B, N] tensor, got %s" % (name, tuple(a.shape) if torch.is_tensor(a) else type(a).__name__))
    B, Na = audio_a.shape
    Nb = audio_b.shape[1]
    if audio_b.shape[0] != B:
        raise ValueError("audio_a holds %d utterances and audio_b %d: one pair per utterance" % (B, audio_b.shape[0]))
    hop = envelope._int_arg(hop_length, "hop_length", 1)
    na = lengths_arg(n_a, "n_a", B, Na) or [Na] * B
    nb = lengths_arg(n_b, "n_b", B, Nb) or [Nb] * B
    al, bl = _pair_lengths([n // hop + 1 for n in na], [n // hop + 1 for n in nb], B, Na // hop + 1, Nb // hop + 1, ("n_a", "n_b"),
                           not align, "align=False")
    mc_a = envelope.mel_cepstra(audio_a, na, f0_a, sampling_rate, hop, order, alpha)
    mc_b = envelope.mel_cepstra(audio_b, nb, f0_b, sampling_rate, hop, order, alpha)
    cost, path, path_len = dtw(mc_a[:, :, 1:], mc_b[:, :, 1:], al, bl, diagonal=not align)
    mcd = (MCD_SCALE * cost.double() / path_len.double()).float()
    return (mcd, path, path_len) if return_path else mcd


def f0_distortion(f0_a, f0_b, path, path_len):
    """F0 error of two pitch contours along a warping path, pair by pair, in one launch: f0_a [B, Ta] and f0_b [B, Tb] in Hz
    with 0 = unvoiced (fp32 on the device, any strides: pitch.f0 of the two waveforms at the mel front end's hop), path
    [B, P, 2] int32 and path_len [B] int32 on the device as dtw() or mel_cepstral_distortion(..., return_path=True) return
    them; cells at or behind path_len[b] are not read.
    -> (rmse_cents [B] fp32: sqrt of the mean of (1200 log2(f0_a[i] / f0_b[j]))^2 over the cells (i, j) where both frames are
    voiced, float64 throughout and rounded to fp32 once, NaN where there is no such cell; vuv_error [B] fp32: the share of
    the path's cells where exactly one frame is voiced; n_voiced [B] int32: the cells where both are).
    The contours are those of THIS project's tracker on Griffin-Lim audio: the numbers compare runs of this model, not papers."""
    for t, name in ((f0_a, "f0_a"), (f0_b, "f0_b")):
        if not torch.is_tensor(t) or t.dim() != 2:
            raise ValueError("%s must be a [B, T] tensor, got %s" % (name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        if min(t.shape) < 1:
            raise ValueError("%s must hold at least one utterance and one frame, got shape %s" % (name, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (name, t.dtype))
    B, Ta = f0_a.shape
    Tb = f0_b.shape[1]
    if f0_b.shape[0] != B:
        raise ValueError("f0_a holds %d contours and f0_b %d: one pair per utterance" % (B, f0_b.shape[0]))
    if not torch.is_tensor(path) or path.dim() != 3 or path.shape[0] != B or path.shape[1] < 1 or path.shape[2] != 2 or path.dtype != torch.int32:
        raise ValueError("path must be a [%d, P, 2] int32 tensor, got %s" % (B, (tuple(path.shape), path.dtype) if torch.is_tensor(path) else type(path).__name__))
    if not torch.is_tensor(path_len) or tuple(path_len.shape) != (B,) or path_len.dtype != torch.int32:
        raise ValueError("path_len must be a [%d] int32 tensor, got %s" % (B, (tuple(path_len.shape), path_len.dtype) if torch.is_tensor(path_len) else type(path_len).__name__))
    if path.shape[1] > Ta + Tb - 1:
        raise ValueError("path has room for %d cells, a warp of %d x %d frames has at most %d: these contours are not the path's" % (path.shape[1], Ta, Tb, Ta + Tb - 1))
    L.require_cuda(f0_a, f0_b, path, path_len)
    n_both, n_mismatch, sum_sq = ops.f0_path_stats(f0_a.detach(), f0_b.detach(), path.contiguous(), path_len.contiguous())
    rmse = torch.sqrt(sum_sq / n_both.double()).float()                     # 0 / 0 = NaN where no cell has both voiced
    vuv = (n_mismatch.double() / path_len.double()).float()
    return rmse, vuv, n_both
