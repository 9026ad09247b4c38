"""NumPy replay of csrc/level.hip in the order include/flowtron_hip.h documents: frame powers, bounds and peak; the three-pass
K-weighting filter; step sums, blocks and gates; the gain; the gather.  The host tables (coefficients, carry matrix, thresholds)
are flowtron_amd.level's own functions.  Everything takes ONE utterance (a float32 vector of its n samples); the batch helpers at
the end loop over utterances -- which is also the statement that an utterance does not depend on its batch."""
import math

import numpy as np

from flowtron_amd import level as LV

CHUNK = LV.CHUNK
_XOR = [np.arange(64) ^ off for off in (32, 16, 8, 4, 2, 1)]


# ---- endpoints ----------------------------------------------------------------------------------------------------------------------

def frame_powers(x, frame_length, hop):
    """x float32 [n] -> float32 [n // hop + 1]: lane l adds the squares of the samples l, l + 64, .. ascending in float64,
    the xor butterfly, one division, one rounding"""
    x = np.asarray(x, np.float32)
    n, F = x.size, frame_length
    T = n // hop + 1
    buf = np.zeros(F // 2 + max(n, (T - 1) * hop + F), np.float64)
    buf[F // 2:F // 2 + n] = x
    frames = buf[(np.arange(T) * hop)[:, None] + np.arange(F)[None, :]]
    sq = np.zeros((T, -(-F // 64) * 64), np.float64)
    sq[:, :F] = frames * frames
    sq = sq.reshape(T, -1, 64)
    q = np.zeros((T, 64), np.float64)
    for k in range(sq.shape[1]):
        q = q + sq[:, k, :]
    for perm in _XOR:
        q = q + q[:, perm]
    return (q[:, 0] / np.float64(F)).astype(np.float32)


def peak(x):
    x = np.asarray(x, np.float32)
    return np.float32(np.max(np.abs(x))) if x.size else np.float32(0)


def bounds(power, n, hop, top_db=60.0, ref="max", pad=0):
    """-> (start, end) from one utterance's frame powers"""
    thr = np.float64(np.float32(LV.threshold_power(top_db)))
    ref_power = np.float64(np.max(power)) if ref == "max" else np.float64(np.float32(ref))
    active = np.nonzero(power.astype(np.float64) > thr * ref_power)[0]
    if active.size == 0:
        return 0, n
    s = max(int(active[0]) * hop - pad, 0)
    e = min((int(active[-1]) + 1) * hop + pad, n)
    return (0, n) if s >= e else (s, e)


def active_bounds(x, top_db=60.0, frame_length=2048, hop=512, ref="max", pad=0):
    return bounds(frame_powers(x, frame_length, hop), len(x), hop, top_db, ref, pad)


# ---- the K-weighting filter as a chunked recurrence -----------------------------------------------------------------------------------

def _run_chunks(x, coef, states, chunk):
    """every chunk of x from its row of states [nc, 4] (v1, v2, y1, y2) -> (end states [nc, 4], outputs [len])"""
    b0, b1, b2, a1, a2, h1, h2 = [np.float64(c) for c in coef]
    n = x.size
    nc = -(-n // chunk)
    X = np.zeros(nc * chunk, np.float64)
    X[:n] = x
    X = X.reshape(nc, chunk)
    valid = (np.arange(nc * chunk) < n).reshape(nc, chunk)
    x1, x2 = np.zeros(nc), np.zeros(nc)
    x1[1:] = X[:-1, chunk - 1]
    x2[1:] = X[:-1, chunk - 2]
    v1, v2, y1, y2 = [states[:, i].copy() for i in range(4)]
    Y = np.zeros((nc, chunk), np.float64)
    for j in range(chunk):
        u = X[:, j]
        v = (((b0 * u + b1 * x1) + b2 * x2) - a1 * v1) - a2 * v2
        y = (((v - 2.0 * v1) + v2) - h1 * y1) - h2 * y2
        m = valid[:, j]
        x2, x1 = np.where(m, x1, x2), np.where(m, u, x1)
        v2, v1 = np.where(m, v1, v2), np.where(m, v, v1)
        y2, y1 = np.where(m, y1, y2), np.where(m, y, y1)
        Y[:, j] = y
    return np.stack([v1, v2, y1, y2], 1), Y.reshape(-1)[:n]


def carry_states(z, M):
    """s[0] = 0, s[c + 1] = z[c] + M s[c], row r as z + (((M0 s0 + M1 s1) + M2 s2) + M3 s3)"""
    s = np.zeros_like(z)
    cur = [0.0, 0.0, 0.0, 0.0]
    for c in range(z.shape[0]):
        s[c] = cur
        cur = [float(z[c, r]) + (((M[r][0] * cur[0] + M[r][1] * cur[1]) + M[r][2] * cur[2]) + M[r][3] * cur[3]) for r in range(4)]
    return s


def k_filter(x, sampling_rate, chunk=CHUNK):
    """x float32 [len] -> the K-weighted signal, float64 [len], by the kernels' three passes"""
    x = np.asarray(x, np.float32)
    coef = LV.filter_coefficients(sampling_rate)
    nc = -(-x.size // chunk)
    z, _ = _run_chunks(x, coef, np.zeros((nc, 4)), chunk)
    s = carry_states(z, LV.carry_matrix(coef, chunk))
    return _run_chunks(x, coef, s, chunk)[1]


def step_sums(y, step, chunk=CHUNK):
    """the squared outputs of every whole step: per (chunk, step) segment ascending from 0, the segments ascending from 0"""
    sq = y * y
    ns = y.size // step
    out = np.zeros(ns, np.float64)
    for k in range(ns):
        a = 0.0
        for c in range(k * step // chunk, ((k + 1) * step - 1) // chunk + 1):
            i0, i1 = max(c * chunk, k * step), min((c + 1) * chunk, (k + 1) * step)
            a = a + np.add.accumulate(sq[i0:i1])[-1]
        out[k] = a
    return out


def gated_power(sums, step):
    nb = max(len(sums) - 3, 0)
    if nb == 0:
        return float("nan")
    den = float(4 * step)
    z = [((float(sums[j]) + float(sums[j + 1])) + (float(sums[j + 2]) + float(sums[j + 3]))) / den for j in range(nb)]
    gate = LV.absolute_gate_power()
    kept = [v for v in z if v > gate]
    if not kept:
        return 0.0
    total = 0.0
    for v in kept:
        total = total + v
    rel = 0.1 * (total / float(len(kept)))
    kept = [v for v in kept if v > rel]
    if not kept:
        return 0.0
    total = 0.0
    for v in kept:
        total = total + v
    return total / float(len(kept))


def lufs_of(power):
    if math.isnan(power):
        return float("nan")
    return LV.LUFS_OFFSET + 10.0 * math.log10(power) if power > 0 else float("-inf")


def loudness(x, sampling_rate, chunk=CHUNK):
    """-> (lufs, power, step sums) of one utterance"""
    step = LV.block_step(sampling_rate)
    sums = step_sums(k_filter(x, sampling_rate, chunk), step, chunk)
    power = gated_power(sums, step)
    return lufs_of(power), power, sums


# ---- gain and gather ------------------------------------------------------------------------------------------------------------------

def gain_for(lufs, pk, target_lufs=-23.0, peak_ceiling=0.99, max_gain_db=30.0):
    cap = 10.0 ** (max_gain_db / 20.0)
    pk = float(pk)
    if target_lufs is None:
        g = 1.0 if peak_ceiling is None or not pk > 0 else peak_ceiling / pk
        g = min(g, cap)
    else:
        g = float(np.power(10.0, (target_lufs - lufs) / 20.0)) if math.isfinite(lufs) else 1.0
        g = min(g, cap)
        if peak_ceiling is not None and g * pk > peak_ceiling:
            g = peak_ceiling / pk
    return np.float32(g)


def gather(x, start, end, N, gain=None):
    """-> float32 [N]: x[start:end] (times the fp32 gain, one rounding) at the front, zeros behind"""
    out = np.zeros(N, np.float32)
    seg = np.asarray(x[start:end], np.float32)
    out[:end - start] = seg if gain is None else np.float32(gain) * seg
    return out


def prepare(x, N, sampling_rate, top_db=60.0, target_lufs=-23.0, peak_ceiling=0.99, max_gain_db=30.0, frame_length=2048, hop=512,
            ref="max", pad=0):
    """one utterance through bounds, loudness of the span, gain, gather -> dict"""
    s, e = active_bounds(x, top_db, frame_length, hop, ref, pad)
    lufs, power, sums = loudness(x[s:e], sampling_rate)
    pk = peak(x[s:e])
    g = gain_for(lufs, pk, target_lufs, peak_ceiling, max_gain_db)
    return dict(start=s, end=e, lufs=lufs, power=power, step_sums=sums, peak=pk, gain=g, out=gather(x, s, e, N, g), n_out=e - s)


# ---- signals --------------------------------------------------------------------------------------------------------------------------

def voice(n, sampling_rate, onset, offset, seed=0, amplitude=0.3):
    """a 140 Hz voice with vibrato and noise whose head [0, onset) and tail [offset, n) are scaled by 1e-4 (an 80 dB step)"""
    rng = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64) / sampling_rate
    phase = 2 * np.pi * 140.0 * t + 0.8 * np.sin(2 * np.pi * 5.5 * t)
    x = amplitude * (np.sin(phase) + 0.4 * np.sin(2 * phase + 0.3) + 0.2 * np.sin(3 * phase + 1.1)) / 1.6 + 0.01 * amplitude * rng.randn(n)
    x[:onset] *= 1e-4
    x[offset:] *= 1e-4
    return x.astype(np.float32)


def tone(n, sampling_rate, freq=997.0, amplitude=1.0):
    return (amplitude * np.sin(2 * np.pi * freq * np.arange(n, dtype=np.float64) / sampling_rate)).astype(np.float32)


def silence(n):
    return np.zeros(n, np.float32)
