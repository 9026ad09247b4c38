"""Restatement of the YIN tracker (include/flowtron_hip.h, F0 tracking; csrc/pitch.hip) and of the F0 error along a path in
plain numpy, written from the rule, and the signals the pitch tests share:

    frame t reads x[t hop - W/2 + j], 0 <= j < W + tau_max + 1, zero outside the utterance; T = n // hop + 1 frames
    d(tau) = sum_{j < W} (x[j] - x[j + tau])^2        tau = 0 .. tau_max + 1; j ascending; sub, mul, add rounded one at a time
    s(tau) = s(tau - 1) + d(tau), s(0) = 0;  d'(0) = 1;  d'(tau) = (d(tau) * tau) / s(tau) where s(tau) > 0, else 1
    tau = the lowest lag in tau_min ..= tau_max with d'(tau) < threshold, then upwards while d'(tau + 1) < d'(tau)
    voiced: a, b, c = d'(tau - 1), d'(tau), d'(tau + 1); den = (a + c) - 2 b; shift = (0.5 (a - c)) / den when a >= b, c >= b and
            den > 0, else 0; f0 = sr / (tau + shift); aperiodicity = b
    unvoiced: f0 = 0, aperiodicity = the least d' in tau_min ..= tau_max

yin(x, cfg, dtype) runs it in float32 (the kernel's arithmetic, so the kernel must give the same bits) or in float64,
vectorised over frames and lags with a loop over j and one over tau for the running sum."""
import math
import warnings

import numpy as np

# sampling rate, hop, window, lags (floor(sr / fmax) .. ceil(sr / fmin)), threshold
DEFAULT = dict(sr=22050.0, hop=256, W=1024, tau_min=55, tau_max=368, threshold=0.15, fmin=60.0, fmax=400.0)
SMALL = dict(sr=8000.0, hop=80, W=256, tau_min=20, tau_max=100, threshold=0.15, fmin=80.0, fmax=400.0)
CONFIGS = {"default": DEFAULT, "small": SMALL}


def with_lags(cfg, **kw):
    return dict(cfg, **kw)


def frames(x, cfg):
    """x [n] -> [T, W + tau_max + 1]: the windows, zero outside the utterance"""
    n, hop, W = len(x), cfg["hop"], cfg["W"]
    span = W + cfg["tau_max"] + 1
    T = n // hop + 1
    pad = np.concatenate([np.zeros(W // 2, x.dtype), x, np.zeros(T * hop + span, x.dtype)])
    return np.stack([pad[t * hop:t * hop + span] for t in range(T)])


def difference(x, cfg, dtype=np.float32):
    """-> (d [T, tau_max + 2], s [T, tau_max + 2]) as dtype"""
    X = frames(np.asarray(x, dtype), cfg)
    nl = cfg["tau_max"] + 2
    d = np.zeros((X.shape[0], nl), dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for j in range(cfg["W"]):
            df = X[:, j:j + 1] - X[:, j:j + nl]
            d = d + df * df
        s = np.zeros_like(d)
        for tau in range(1, nl):
            s[:, tau] = s[:, tau - 1] + d[:, tau]
    return d, s


def normalised(d, s):
    """-> d' [T, tau_max + 2] in the dtype of d"""
    dtype = d.dtype.type
    tau = np.arange(d.shape[1]).astype(dtype)[None, :]
    ok = s > 0
    ok[:, 0] = False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.where(ok, (d * tau) / np.where(ok, s, dtype(1)), dtype(1)).astype(dtype)


def yin(x, cfg, dtype=np.float32, details=False):
    """x [n] -> (f0 [T], aperiodicity [T]) as dtype; details: also (lag [T] int, 0 = unvoiced; d; s)"""
    x = np.asarray(x, dtype)
    dtype = x.dtype.type
    d, s = difference(x, cfg, dtype)
    dp = normalised(d, s)
    lo, hi, thr, sr = cfg["tau_min"], cfg["tau_max"], dtype(np.float32(cfg["threshold"])), dtype(np.float32(cfg["sr"]))
    T = d.shape[0]
    f0, ap, lag = np.zeros(T, dtype), np.zeros(T, dtype), np.zeros(T, np.int64)
    bad = ~np.isfinite(frames(x, cfg)).all(1)
    for t in range(T):
        row = dp[t]
        below = np.nonzero(row[lo:hi + 1] < thr)[0]
        if bad[t]:
            f0[t], ap[t] = 0, 1                   # the aperiodicity of such a frame is unspecified: the kernel's choice
            continue
        if len(below) == 0:
            ap[t] = row[lo:hi + 1].min()
            continue
        tau = lo + int(below[0])
        while tau < hi and row[tau + 1] < row[tau]:
            tau += 1
        a, b, c = row[tau - 1], row[tau], row[tau + 1]
        den = dtype(dtype(a + c) - dtype(dtype(2) * b))
        shift = dtype(0)
        if a >= b and c >= b and den > 0:
            shift = dtype(dtype(dtype(0.5) * dtype(a - c)) / den)
        f0[t] = dtype(sr / dtype(dtype(tau) + shift))
        ap[t] = b
        lag[t] = tau
    return (f0, ap, lag, d, s) if details else (f0, ap)


# ---- signals ------------------------------------------------------------------------------------------------------------
def tone(n, cfg, seed):
    """-> (x [n] float32, f0 Hz): four harmonics of a constant F0 in 100 .. 250 Hz, amplitude 0.3"""
    rng = np.random.RandomState(seed)
    f = float(rng.uniform(100.0, 250.0))
    t = np.arange(n, dtype=np.float64) / cfg["sr"]
    ph = rng.uniform(0, 2 * np.pi, 4)
    x = sum(np.sin(2 * np.pi * f * (h + 1) * t + ph[h]) / (h + 1) for h in range(4))
    return (0.3 * x / np.abs(x).max()).astype(np.float32), f


def voice(n, cfg, seed):
    """an F0 gliding up by 0.4 octaves a second with six harmonics and 1 % noise; the fourth fifth of it noise only, the last
    tenth exact zeros"""
    rng = np.random.RandomState(seed)
    f = rng.uniform(110.0, 180.0) * 2.0 ** (0.4 * np.arange(n) / cfg["sr"])
    ph = 2 * np.pi * np.cumsum(f) / cfg["sr"]
    x = 0.3 * sum(np.sin((h + 1) * ph) / (h + 1) for h in range(6)) / 2.0 + 0.01 * rng.randn(n)
    a, b, c = (3 * n) // 5, (4 * n) // 5, n - n // 10
    x[a:b] = 0.05 * rng.randn(b - a)
    x[c:] = 0.0
    return x.astype(np.float32)


def grid(n, cfg, seed):
    """-> (x [n] float32, period): a periodic signal with an integer period inside the lag range, integer multiples of 2^-6 of
    magnitude at most 3 * 2^-6.  A squared difference is then at most 36 units of 2^-12, d at most 36 W and s at most
    36 W (tau_max + 1) of them: below 2^24 at both configurations, so every sum is exact in float32 and in float64"""
    rng = np.random.RandomState(seed)
    period = int(rng.randint(cfg["tau_min"] + 2, min(cfg["tau_max"] // 2, 2 * cfg["tau_min"] + 8)))
    one = rng.randint(-3, 4, period).astype(np.float32) / np.float32(64)
    return np.tile(one, n // period + 1)[:n].copy(), period


def signal(kind, n, cfg, seed):
    if kind == "tone":
        return tone(n, cfg, seed)[0]
    if kind == "voice":
        return voice(n, cfg, seed)
    return grid(n, cfg, seed)[0]


# ---- F0 error along a path ----------------------------------------------------------------------------------------------
def path_stats(fa, fb, path):
    """float64 statement: fa [Ta], fb [Tb] Hz (0 = unvoiced), path [P, 2] -> (n_both, n_mismatch, sum of squared cents)"""
    n_both = n_mis = 0
    total = 0.0
    for i, j in np.asarray(path).tolist():
        a, b = float(fa[i]), float(fb[j])
        if a > 0 and b > 0:
            total += (1200.0 * math.log2(a / b)) ** 2
            n_both += 1
        elif (a > 0) != (b > 0):
            n_mis += 1
    return n_both, n_mis, total


def distortion(fa, fb, path):
    """-> (rmse_cents float32, NaN without a both-voiced cell; vuv_error float32; n_voiced)"""
    n_both, n_mis, total = path_stats(fa, fb, path)
    rmse = np.float32(math.sqrt(total / n_both)) if n_both else np.float32("nan")
    return rmse, np.float32(n_mis / len(path)), n_both


def statistics(f0):
    """-> (n voiced, mean, std) of 12 log2(f0) over the voiced frames in float64, NaN where nothing is voiced"""
    v = np.asarray(f0, np.float64)
    v = v[v > 0]
    if len(v) == 0:
        return 0, float("nan"), float("nan")
    st = 12.0 * np.log2(v)
    return len(v), float(st.mean()), float(st.std())
