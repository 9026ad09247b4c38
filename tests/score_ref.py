"""NumPy replays of csrc/score.hip as include/flowtron_hip.h states the two rules.  TEST INFRASTRUCTURE.
frame_loglik: float64 in the documented order (lanes own the channels l and l + 64, xor butterfly over the 64 lanes, totals from
256 strided partial sums and a halving tree), every operation rounded on its own -- NumPy never fuses a multiply and an add.
attn_diagnostics: a float32 arg-max with the kernel's tie and NaN rule, then plain integer logic."""
import math

import numpy as np

COUNTERS = ("n_attended", "n_backward", "n_skipped", "longest_run", "first_peak", "last_peak")


def _butterfly(v):
    """v [..., 64] -> the value every lane holds after v_l = v_l + v_{l ^ off}, off = 32 .. 1"""
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ off]
    return v[..., 0]


def host_constants(M, sigma):
    """(inv, c) as ft_frame_loglik forms them on the host"""
    sigma = float(sigma)
    return 1.0 / (2.0 * sigma * sigma), M * 0.5 * math.log(6.283185307179586 * sigma * sigma)


def frame_loglik(z, log_s, reversed_, out_lens, sigma=1.0):
    """z [T, B, M] float32, log_s: list of [T, B, M] float32 (any strides), reversed_: list of flags, out_lens [B]
    -> (frame_ll [B, T] float64, total [B] float64) with the kernel's bits"""
    T, B, M = z.shape
    assert 1 <= M <= 128 and z.dtype == np.float32 and all(ls.dtype == np.float32 for ls in log_s)
    inv, c = host_constants(M, sigma)
    frame_ll = np.zeros((B, T), np.float64)
    total = np.zeros(B, np.float64)
    for b in range(B):
        n = min(max(int(out_lens[b]), 0), T)
        if n:
            def lanes(x):                                          # [n, M] float32 -> the two channels of every lane, [n, 2, 64] float64
                pad = np.zeros((n, 128), np.float64)
                pad[:, :M] = x.astype(np.float64)
                return pad.reshape(n, 2, 64)
            zz = lanes(z[:n, b])
            q = (0.0 + zz[:, 0] * zz[:, 0])
            q = np.where(np.arange(64)[None, :] + 64 < M, q + zz[:, 1] * zz[:, 1], q)
            q = np.where(np.arange(64)[None, :] < M, q, 0.0)
            s = np.zeros((n, 64), np.float64)
            for ls, rev in zip(log_s, reversed_):
                x = ls[:n, b]
                if rev:
                    x = x[::-1]
                xx = lanes(x)
                s = np.where(np.arange(64)[None, :] < M, s + xx[:, 0], s)
                s = np.where(np.arange(64)[None, :] + 64 < M, s + xx[:, 1], s)
            Q, S = _butterfly(q), _butterfly(s)
            frame_ll[b, :n] = ((-(Q * inv)) - c) + S
        part = np.zeros(256, np.float64)
        for t0 in range(0, n, 256):
            chunk = frame_ll[b, t0:min(t0 + 256, n)]
            part[:len(chunk)] = part[:len(chunk)] + chunk
        h = 128
        while h:
            part[:h] = part[:h] + part[h:2 * h]
            h //= 2
        total[b] = part[0]
    return frame_ll, total


def frame_loglik_brute(z, log_s, reversed_, out_lens, sigma=1.0):
    """the definition, straight: float64, numpy's own summation order"""
    T, B, M = z.shape
    frame_ll = np.zeros((B, T), np.float64)
    for b in range(B):
        n = min(max(int(out_lens[b]), 0), T)
        for t in range(n):
            v = -np.sum(z[t, b].astype(np.float64) ** 2) / (2.0 * sigma * sigma) - 0.5 * M * math.log(2.0 * math.pi * sigma * sigma)
            for ls, rev in zip(log_s, reversed_):
                v += np.sum(ls[n - 1 - t if rev else t, b].astype(np.float64))
            frame_ll[b, t] = v
    return frame_ll, frame_ll.sum(1)


def peak_of(row):
    """row [l] float32 -> (peak, pmax): the lowest index whose value is largest, replacing only on `>` from -inf"""
    above = row > -np.inf                                          # (False for NaN)
    if not above.any():
        return 0, row[0]
    m = row[above].max()
    j = int(np.flatnonzero(row == m)[0])
    return j, row[j]


def counters_of(peaks):
    """peaks [n] ints -> dict of the six counters"""
    p = [int(x) for x in peaks]
    run = best = 1
    for a, b in zip(p, p[1:]):
        run = run + 1 if a == b else 1
        best = max(best, run)
    return dict(n_attended=len(set(p)), n_backward=sum(b < a for a, b in zip(p, p[1:])),
                n_skipped=sum(max(b - a - 1, 0) for a, b in zip(p, p[1:])), longest_run=best, first_peak=p[0], last_peak=p[-1])


def attn_diagnostics(attn, in_lens, out_lens):
    """attn [F, B, T, L] float32 (natural time) -> (peaks [F, B, T] int32 with -1 behind n, counters [F, B, 6] int32,
    focus_sum [F, B] float64 in the kernel's order: 16 waves take the frames w, w + 16, .., their sums are added in wave order)"""
    F, B, T, L = attn.shape
    peaks = np.full((F, B, T), -1, np.int32)
    counters = np.zeros((F, B, 6), np.int32)
    focus = np.zeros((F, B), np.float64)
    for f in range(F):
        for b in range(B):
            n, l = min(max(int(out_lens[b]), 1), T), min(max(int(in_lens[b]), 1), L)
            part = np.zeros(16, np.float64)
            for t in range(n):
                j, v = peak_of(attn[f, b, t, :l])
                peaks[f, b, t] = j
                part[t % 16] = part[t % 16] + np.float64(v)
            fs = np.float64(0.0)
            for w in range(16):
                fs = fs + part[w]
            focus[f, b] = fs
            c = counters_of(peaks[f, b, :n])
            counters[f, b] = [c[k] for k in COUNTERS]
    return peaks, counters, focus


def peak_brute(row):
    """the sequential definition: scan from j = 0, replace only on `>`"""
    best, at = np.float32(-np.inf), 0
    for j, v in enumerate(row):
        if v > best:
            best, at = v, j
    return at, row[at]
