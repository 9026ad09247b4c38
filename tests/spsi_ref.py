"""Host restatement of ft_spsi_phase (csrc/vocode.hip), independent of flowtron_amd.audio: the rule of include/flowtron_hip.h
operation by operation in `dtype`.  numpy rounds every float32 ufunc once and fuses nothing, so `spsi32` gives the kernel's
bits; `spsi64` is the same rule in float64 (for the quality tests).  A frame is handled as a vector over the bins, the frames in
a Python loop, as the accumulator demands."""
import numpy as np


def owners(m):
    """One frame's magnitudes [K] -> (peak [K] bool, owner [K] int, -1 = none): the nearest stop of a strictly ascending walk
    to the right (or, for a bin that does not ascend to the right, to the left) owns the bin if it is a peak."""
    K = len(m)
    idx = np.arange(K)
    asc, desc, peak = np.zeros(K, bool), np.zeros(K, bool), np.zeros(K, bool)
    with np.errstate(invalid="ignore"):
        asc[:-1] = m[:-1] < m[1:]                                  # below the right neighbour
        desc[1:] = m[1:] < m[:-1]                                  # below the left neighbour
        peak[1:-1] = (m[1:-1] > m[:-2]) & (m[1:-1] > m[2:])
    stop_r = np.minimum.accumulate(np.where(~asc, idx, K)[::-1])[::-1]     # the first q >= j that does not ascend (K - 1 never does)
    stop_l = np.maximum.accumulate(np.where(~desc, idx, -1))               # the last q <= j that does not descend leftwards (0 never does)
    owner = np.full(K, -1)
    owner[peak] = idx[peak]
    right = asc & ~peak
    owner[right] = np.where(peak[stop_r[right]], stop_r[right], -1)
    left = ~asc & desc & ~peak
    owner[left] = np.where(peak[stop_l[left]], stop_l[left], -1)
    return peak, owner


def increments(m, peak, n_fft, hop, dtype):
    """inc [K] in turns at the peaks of one frame (0 elsewhere)."""
    K = len(m)
    k = np.nonzero(peak)[0]
    a, b, c = m[k - 1], m[k], m[k + 1]
    with np.errstate(all="ignore"):
        den = (a - b) + (c - b)
        p = (dtype(0.5) * (a - c)) / den
        p = np.where(np.abs(p) <= dtype(0.5), p, dtype(0)).astype(dtype)
    base = ((hop * k) % n_fft).astype(dtype) / dtype(n_fft)
    inc = np.zeros(K, dtype)
    inc[k] = base + (dtype(hop) / dtype(n_fft)) * p
    return inc


def spsi(M, n_fft, hop, dtype, n_frames=None, turns=False):
    """M [B, K, T] or [K, T] magnitudes -> angles of the same shape in `dtype`, 0 at and behind n_frames[b]; turns=True returns
    the accumulator itself (turns) instead of 6.2831855f times it."""
    M = np.asarray(M)
    M3 = (M if M.ndim == 3 else M[None]).astype(dtype)
    B, K, T = M3.shape
    assert K == n_fft // 2 + 1
    two_pi = dtype(np.float32(6.2831855))
    out = np.zeros((B, K, T), dtype)
    jj = np.arange(K)
    for b in range(B):
        n = T if n_frames is None else min(max(int(n_frames[b]), 0), T)
        acc = np.zeros(K, dtype)
        for t in range(n):
            m = M3[b, :, t]
            peak, owner = owners(m)
            inc = increments(m, peak, n_fft, hop, dtype)
            new = acc.copy()
            pk = np.nonzero(peak)[0]
            v = acc[pk] + inc[pk]
            new[pk] = v - np.rint(v)
            own = np.nonzero((owner >= 0) & ~peak)[0]
            k = owner[own]
            w = new[k] + np.where((own - k) & 1, dtype(0.5), dtype(0.0)).astype(dtype)
            new[own] = w - np.rint(w)
            assert new.dtype == dtype
            acc = new
            out[b, :, t] = acc if turns else two_pi * acc
    assert out.dtype == dtype
    return out if M.ndim == 3 else out[0]


def spsi32(M, n_fft, hop, n_frames=None, turns=False):
    return spsi(M, n_fft, hop, np.float32, n_frames, turns)


def spsi64(M, n_fft, hop, n_frames=None, turns=False):
    return spsi(M, n_fft, hop, np.float64, n_frames, turns)
