"""Restatement of probabilistic YIN (include/flowtron_hip.h, F0 through noise; csrc/pitch.hip) in plain numpy, written from the
rule, with its host-side tables, and the noisy glide the accuracy conditions are stated on.  d, s and d' come from
tests/pitch_ref.py.

    n(v) = how many of the thresholds float(i) / 100, i = 1 .. 100, lie at or below v
    trough: d'(tau) <= d'(tau - 1) and d'(tau) < d'(tau + 1), tau_min <= tau <= tau_max
    candidate: a trough lower than every earlier one (rec, +inf at first): w = cum[n(rec)] - cum[n(d'(tau))]
    global minimum (the lowest lag of equals): w = absolute_min_prob * cum[n(d')]
    entry -> lag L = tau + parabolic shift, frequency sr / L, the bin k with edges[k + 1] < L <= edges[k]; w <= 0 and lags
    outside the bins are dropped; prob[k] = sum of w in lag order, the global minimum last; freq[k] = the heaviest entry's
    voiced = 64 strided partial sums of prob, then a halving tree
    Viterbi over (bin, voicing): r_t = ((max over the band of r_{t-1} * transition, times stay or switch) * scale_{t-1}) * obs,
    0 below 2^-64; scale = the power of two that brings the frame's maximum into [1, 2); ties: the lowest offset, keeping the
    voicing, the lowest final state 2 k + x

candidates() / viterbi() / track() run it in float32 (the kernels' arithmetic and the kernels' rounded tables: the same bits)
or in float64 (unrounded tables)."""
import numpy as np

import pitch_ref as R

FLOOR = 2.0 ** -20
CUT = 2.0 ** -64
SETTINGS = dict(bps=10, beta=(2.0, 18.0), amp=0.01, max_octaves=35.92, switch=0.01)


def config(name, **kw):
    """a configuration of pitch_ref with the tracker's settings: 'small' has 279 bins and a band of 43, 'default' 329 and 50"""
    return dict(R.CONFIGS[name], **dict(SETTINGS, **kw))


def beta_cum(a, b):
    """[101] float64: the Beta(a, b) distribution function at i / 100, by Gauss-Legendre quadrature of the density on each
    hundredth (a, b >= 1: the integrand is smooth)"""
    u, w = np.polynomial.legendre.leggauss(48)
    pieces = []
    for i in range(100):
        x = (i + 0.5 + 0.5 * u) / 100.0
        pieces.append(float(np.sum(w * x ** (a - 1.0) * (1.0 - x) ** (b - 1.0))))
    c = np.concatenate([[0.0], np.cumsum(pieces)])
    return c / c[-1]


def n_bins(cfg):
    return int(np.floor(12 * cfg["bps"] * np.log2(cfg["fmax"] / cfg["fmin"]))) + 1


def band(cfg):
    return int(np.floor(cfg["max_octaves"] * 12 * cfg["bps"] * cfg["hop"] / cfg["sr"] + 0.5))


def tables(cfg, dtype=np.float32):
    """-> dict(cum [101], edges [n_bins + 1] descending lags, centres [n_bins] Hz, tri [2 band + 1]) as dtype, formed in
    float64 and rounded once"""
    nb, bd, step = n_bins(cfg), band(cfg), 12.0 * cfg["bps"]
    i = np.arange(nb + 1, dtype=np.float64)
    o = np.arange(2 * bd + 1, dtype=np.float64)
    return dict(cum=beta_cum(*cfg["beta"]).astype(dtype),
                edges=(cfg["sr"] / (cfg["fmin"] * 2.0 ** ((i - 0.5) / step))).astype(dtype),
                centres=(cfg["fmin"] * 2.0 ** (i[:-1] / step)).astype(dtype),
                tri=((bd + 1 - np.abs(o - bd)) / float((bd + 1) ** 2)).astype(dtype))


def _lag(row, tau, dtype):
    a, b, c = row[tau - 1], row[tau], row[tau + 1]
    den = dtype(dtype(a + c) - dtype(dtype(2) * b))
    shift = dtype(0)
    if a >= b and c >= b and den > 0:
        shift = dtype(dtype(dtype(0.5) * dtype(a - c)) / den)
    return dtype(dtype(tau) + shift)


def voiced_sum(prob, dtype):
    """prob [T, n_bins] -> [T]: p[l] = prob[l] + prob[l + 64] + .., then p[l] += p[l + h] for h = 32 .. 1"""
    T, nb = prob.shape
    rows = np.zeros((T, -(-nb // 64) * 64), dtype)
    rows[:, :nb] = prob
    rows = rows.reshape(T, -1, 64)
    p = np.zeros((T, 64), dtype)
    for r in range(rows.shape[1]):
        p = p + rows[:, r]
    h = 32
    while h:
        p = p[:, :h] + p[:, h:2 * h]
        h //= 2
    return p[:, 0]


def candidates(x, cfg, dtype=np.float32, tab=None):
    """x [n] -> (prob [T, n_bins], freq [T, n_bins], voiced [T]) as dtype"""
    x = np.asarray(x, dtype)
    dtype = x.dtype.type
    tab = tab or tables(cfg, dtype)
    cum, edges = tab["cum"], tab["edges"]
    nb = len(edges) - 1
    d, s = R.difference(x, cfg, dtype)
    dp = R.normalised(d, s)
    lo, hi, sr, amp = cfg["tau_min"], cfg["tau_max"], dtype(np.float32(cfg["sr"])), dtype(np.float32(cfg["amp"]))
    thr = np.arange(1, 101).astype(dtype) / dtype(100)
    bad = ~np.isfinite(R.frames(x, cfg)).all(1)
    T = d.shape[0]
    prob, freq = np.zeros((T, nb), dtype), np.zeros((T, nb), dtype)

    def count(v):
        return int(np.searchsorted(thr, v, side="right"))

    def which_bin(lag):
        if not lag <= edges[0] or not lag > edges[nb]:
            return -1
        return int(np.nonzero(edges[:nb] >= lag)[0][-1])          # descending: the last edge at or above the lag

    for t in range(T):
        row = dp[t]
        if bad[t] or not s[t, hi + 1] > 0:
            continue
        entries = []                                               # (weight, lag)
        rec, least, glag = np.inf, np.inf, None
        for tau in range(lo, hi + 1):
            v = row[tau]
            if v <= row[tau - 1] and v < row[tau + 1] and v < rec:
                entries.append((dtype(cum[count(rec)] - cum[count(v)]), _lag(row, tau, dtype)))
                rec = v
            if v < least:
                least, glag = v, tau
        if glag is not None:
            entries.append((dtype(amp * cum[count(least)]), _lag(row, glag, dtype)))
        heaviest = np.zeros(nb, dtype)
        for w, lag in entries:
            k = which_bin(lag) if w > 0 else -1
            if k < 0:
                continue
            prob[t, k] = prob[t, k] + w
            if w > heaviest[k]:
                heaviest[k], freq[t, k] = w, dtype(sr / lag)
    return prob, freq, voiced_sum(prob, dtype)


def viterbi(prob, freq, voiced, cfg, tab=None):
    """-> (f0 [T] in the dtype of prob, states [T] int: 2 k + x, x = 1 voiced)"""
    dtype = prob.dtype.type
    tab = tab or tables(cfg, dtype)
    tri, centres = tab["tri"], tab["centres"]
    T, nb = prob.shape
    bd = (len(tri) - 1) // 2
    sw = dtype(np.float32(cfg["switch"]))
    stay = dtype(dtype(1) - sw)
    floor, cut = dtype(FLOOR), dtype(CUT)
    back = np.zeros((T, 2, nb, 2), np.int64)                       # (offset, voicing) of the predecessor
    r = None
    for t in range(T):
        u = dtype(dtype(1) - voiced[t])
        u = dtype(0) if u < 0 else u
        obs = np.stack([np.full(nb, dtype(u / dtype(nb)), dtype), prob[t]])        # [voicing, bin]
        obs = np.where(obs < floor, floor, obs)
        if t == 0:
            r = obs
            continue
        m = r.max()
        scale = dtype(np.ldexp(1.0, 1 - int(np.frexp(m)[1])))      # m = f 2^ex, f in [0.5, 1): 2^e <= m < 2^(e + 1) with e = ex - 1
        pad = np.zeros((2, nb + 2 * bd), dtype)
        pad[:, bd:bd + nb] = r
        A = pad[:, 0:nb] * tri[0]
        bo = np.zeros((2, nb), np.int64)
        for o in range(1, 2 * bd + 1):
            c = pad[:, o:o + nb] * tri[o]
            better = c > A
            A = np.where(better, c, A)
            bo = np.where(better, o, bo)
        keep, chg = A * stay, A[::-1] * sw
        change = chg > keep
        own = np.array([[0], [1]])
        back[t, :, :, 0] = np.where(change, bo[::-1], bo)
        back[t, :, :, 1] = np.where(change, 1 - own, own)
        r = (np.where(change, chg, keep) * scale) * obs
        r = np.where(r < cut, dtype(0), r).astype(dtype)
    j = int(np.argmax(r.T.reshape(-1)))                            # state 2 k + x: the lowest of equals
    states = np.zeros(T, np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = j
        if t:
            o, px = back[t, j & 1, j >> 1]
            j = 2 * min(max((j >> 1) + int(o) - bd, 0), nb - 1) + int(px)
    k = states >> 1
    f = freq[np.arange(T), k]
    f0 = np.where(states & 1, np.where(f > 0, f, centres[k]), dtype(0)).astype(dtype)
    return f0, states


def track(x, cfg, dtype=np.float32):
    """x [n] -> dict(prob, freq, voiced, f0, states)"""
    x = np.asarray(x, dtype)
    tab = tables(cfg, x.dtype.type)
    prob, freq, voiced = candidates(x, cfg, x.dtype.type, tab)
    f0, states = viterbi(prob, freq, voiced, cfg, tab)
    return dict(prob=prob, freq=freq, voiced=voiced, f0=f0, states=states)


# ---- the accuracy conditions ---------------------------------------------------------------------------------------------
GLIDE_SR, GLIDE_N, GLIDE_HOP = 8000, 8000, 80


def noisy_glide(sigma, seed):
    """-> (x [8000] float32, truth [101] Hz, truly voiced [101] bool) at 8 kHz: 140 Hz gliding up by 0.3 octaves a second with a
    5.5 Hz vibrato, five harmonics, 0.2 s of silence in the middle, white noise of deviation sigma over all of it"""
    sr, n = GLIDE_SR, GLIDE_N
    rng = np.random.RandomState(seed)
    t = np.arange(n) / sr
    f = 140.0 * 2.0 ** (0.3 * t + 0.03 * np.sin(2 * np.pi * 5.5 * t))
    phase = 2 * np.pi * np.cumsum(f) / sr
    ph = [rng.uniform(0, 6.28) for _ in range(5)]
    x = 0.15 * sum(np.sin(h * phase + ph[h - 1]) / h for h in range(1, 6))
    x[3200:4800] = 0.0
    x = x + sigma * rng.randn(n)
    at = np.arange(n // GLIDE_HOP + 1) * GLIDE_HOP                 # the frames' centres; the last one is sample n
    ta = at / sr
    truth = 140.0 * 2.0 ** (0.3 * ta + 0.03 * np.sin(2 * np.pi * 5.5 * ta))
    return x.astype(np.float32), truth, ~((at >= 3200) & (at < 4800))


def score(f0, truth, voiced):
    """-> dict(missed, false_voiced, gross: both-voiced frames more than 100 cents off, rms: cents over the both-voiced frames,
    found: truly voiced frames given a pitch)"""
    f0 = np.asarray(f0, np.float64)
    on = f0 > 0
    both = on & voiced
    cents = 1200.0 * np.log2(f0[both] / truth[both])
    return dict(missed=int((voiced & ~on).sum()), false_voiced=int((on & ~voiced).sum()), gross=int((np.abs(cents) > 100).sum()),
                rms=float(np.sqrt(np.mean(cents ** 2))) if both.any() else float("nan"), found=int(both.sum()))


def check_conditions(sigma, got, yin):
    """The accuracy conditions on score() of the tracker and of plain YIN on the same noisy glide (seeds 1 and 2): caps with margin
    over what the float64 replay gives (tests/test_pyin_cpu.py has its figures), and two strict comparisons against plain YIN."""
    assert sigma in (0.05, 0.10)
    assert got["false_voiced"] <= 6, got                           # the frames at the gap's edges, whose window still holds voiced samples
    assert got["gross"] == 0, got
    if sigma == 0.05:
        assert got["missed"] <= 4, got
        assert got["rms"] <= 20.0, got
        assert yin["missed"] >= 2 * got["missed"], (got, yin)
    else:
        assert got["missed"] <= 25, got
        assert 2 * yin["found"] < got["found"], (got, yin)
