"""NumPy replay of the pitch-synchronous overlap-add rule (include/flowtron_hip.h, pitch and pace of audio; csrc/prosody.hip),
written from the rule, and the signal and the two measures the prosody tests share.  Everything takes ONE utterance.

    per[t]  = clamp(rint((sr 256) / f0[t]), 16 Q, 1024 Q) on a voiced frame, unvoiced_period Q otherwise        (Q = 256)
    step[t] = max(8 Q, rint(float(per[t]) / ratio[t])) on a voiced frame, per[t] otherwise
    frame(p) = min(T - 1, ((p >> 8) + hop / 2) / hop)
    a_0 = 0, a_{k+1} = a_k + per[frame(a_k)] while (a_k >> 8) < n
    s_0 = 0, while (s_j >> 8) < n_out: ta = (s_j pq) >> 16; k advances while k + 1 < K and |a_{k+1} - ta| <= |a_k - ta|;
             src_j = k, half_j = (per[frame(a_k)] + 128) >> 8, s_{j+1} = s_j + step[frame(ta)]
    out[o] = (sum_j w x[m_j + d]) / (sum_j w) over the grains with |d| < half_j, d = o - c_j, ascending j, w = H[(|d| 1024) / half_j]

marks() / synth() / modify() run it in float32 (the kernels' arithmetic: the same bits) or in float64; the positions are
integers in both.  The host-side pieces (the window table, the pace in 1/65536, the default unvoiced period) are
flowtron_amd.prosody's own functions."""
import numpy as np

from flowtron_amd import prosody as PR

Q = 256


def _periods(f0, ratio, sr, unvoiced_period, dtype):
    """-> (per [T], step [T]) int64"""
    f = np.asarray(f0, dtype)
    T = len(f)
    r = np.broadcast_to(np.asarray(ratio, dtype), (T,)).astype(dtype)
    r = np.where(r >= dtype(PR.MIN_RATIO), r, dtype(PR.MIN_RATIO))
    r = np.where(r <= dtype(PR.MAX_RATIO), r, dtype(PR.MAX_RATIO)).astype(dtype)
    voiced = np.isfinite(f) & (f > 0)
    sr256 = dtype(np.float32(sr * 256.0)) if dtype == np.float32 else dtype(sr * 256.0)
    with np.errstate(all="ignore"):
        q = np.rint((sr256 / np.where(voiced, f, dtype(1))).astype(dtype))
        q = np.minimum(np.maximum(q, dtype(16 * Q)), dtype(1024 * Q))
        per = np.where(voiced, q, dtype(unvoiced_period * Q)).astype(np.int64)
        st = np.rint((per.astype(dtype) / r).astype(dtype)).astype(np.int64)
    step = np.where(voiced, np.maximum(st, 8 * Q), per)
    return per, step


def marks(f0, n, sr, hop, ratio=1.0, pace=1.0, unvoiced_period=None, dtype=np.float32):
    """f0 [T] Hz of ONE utterance of n samples -> dict(analysis [K], synthesis [J], source [J], half [J] int32, n_out)"""
    dtype = np.dtype(dtype).type
    T = len(f0)
    assert T >= n // hop + 1
    unv = PR.default_unvoiced_period(sr) if unvoiced_period is None else int(unvoiced_period)
    per, step = _periods(f0, ratio, sr, unv, dtype)
    per, step = per.tolist(), step.tolist()
    pq = PR.pace_q(pace)
    n_out = max(1, (n << 16) // pq)

    def frame(p):
        return min(T - 1, ((p >> 8) + hop // 2) // hop)

    a = [0]
    while True:
        nxt = a[-1] + per[frame(a[-1])]
        if (nxt >> 8) >= n:
            break
        a.append(nxt)
    K = len(a)
    s, syn, src, half, k = 0, [], [], [], 0
    while (s >> 8) < n_out:
        ta = (s * pq) >> 16
        while k + 1 < K and abs(a[k + 1] - ta) <= abs(a[k] - ta):
            k += 1
        syn.append(s)
        src.append(k)
        half.append((per[frame(a[k])] + 128) >> 8)
        s += step[frame(ta)]
    i32 = lambda v: np.asarray(v, np.int32)
    return dict(analysis=i32(a), synthesis=i32(syn), source=i32(src), half=i32(half), n_out=n_out)


def synth(x, m, dtype=np.float32):
    """x [n] and marks() of it -> out [n_out] as dtype, every multiplication and addition rounded on its own"""
    dtype = np.dtype(dtype).type
    x = np.asarray(x, dtype)
    n, n_out = len(x), m["n_out"]
    H = PR.hann_table().astype(dtype)
    y, ws = np.zeros(n_out, dtype), np.zeros(n_out, dtype)
    c = (m["synthesis"].astype(np.int64) + 128) >> 8
    mm = (m["analysis"].astype(np.int64)[m["source"]] + 128) >> 8
    for cj, mj, h in zip(c.tolist(), mm.tolist(), m["half"].tolist()):
        lo, hi = max(cj - h + 1, 0), min(cj + h, n_out)                     # |o - c_j| < half_j
        if lo >= hi:
            continue
        d = np.arange(lo, hi) - cj
        w = H[(np.abs(d) * 1024) // h]
        i = mj + d
        ok = (i >= 0) & (i < n)
        xv = np.where(ok, x[np.clip(i, 0, n - 1)], dtype(0)).astype(dtype)
        ws[lo:hi] = ws[lo:hi] + w
        y[lo:hi] = y[lo:hi] + (w * xv).astype(dtype)
    ok = ws >= dtype(2.0 ** -10)
    with np.errstate(all="ignore"):
        return np.where(ok, y / np.where(ok, ws, dtype(1)), dtype(0)).astype(dtype)


def modify(x, f0, sr, hop, ratio=1.0, pace=1.0, unvoiced_period=None, dtype=np.float32):
    """-> (out [n_out], marks)"""
    m = marks(f0, len(x), sr, hop, ratio, pace, unvoiced_period, dtype)
    return synth(x, m, dtype), m


def pitch_ratio(f0, shift_semitones=0.0, range_scale=1.0):
    """float64 statement of prosody.pitch_ratio for one utterance -> [T] float32"""
    f = np.asarray(f0, np.float64)
    v = f > 0
    lf = np.log2(np.where(v, f, 1.0))
    mean = lf[v].mean() if v.any() else 0.0
    target = mean + range_scale * (lf - mean) + shift_semitones / 12.0
    return np.where(v, 2.0 ** (target - lf), 1.0).astype(np.float32)


# ---- the shared signal -----------------------------------------------------------------------------------------------------------
SR, N, HOP = 8000, 8000, 80
GAP = (3200, 4800)


def glide_f0(t):
    """the F0 in Hz at t seconds: 140 Hz gliding up by 0.3 octaves a second with a 5.5 Hz vibrato of 0.03 octaves"""
    t = np.asarray(t, np.float64)
    return 140.0 * 2.0 ** (0.3 * t + 0.03 * np.sin(2 * np.pi * 5.5 * t))


def env(f):
    """the spectral envelope every harmonic's amplitude is read from: two resonances, 600 and 1700 Hz, over a floor"""
    f = np.asarray(f, np.float64)
    return 1.0 / np.sqrt(1.0 + ((f - 600.0) / 150.0) ** 2) + 0.6 / np.sqrt(1.0 + ((f - 1700.0) / 250.0) ** 2) + 0.02


def pulse_glide(seed):
    """-> (x [8000] float32, truth [101] Hz at the frames' centres, truly voiced [101] bool) at 8 kHz: harmonics 1 .. 25 below
    3600 Hz of glide_f0 with the amplitudes of env and the phases of its two resonances (pulse-like), peak 0.3, 0.2 s of
    silence in the middle, white noise of deviation 0.005 over all of it"""
    rng = np.random.RandomState(seed)
    t = np.arange(N) / SR
    f = glide_f0(t)
    phase = 2 * np.pi * np.cumsum(f) / SR
    x = np.zeros(N)
    for h in range(1, 26):
        hf = h * f
        ph = -np.arctan((hf - 600.0) / 150.0) - np.arctan((hf - 1700.0) / 250.0)
        x += np.where(hf < 3600.0, env(hf) * np.cos(h * phase + ph), 0.0)
    x *= 0.3 / np.abs(x).max()
    x[GAP[0]:GAP[1]] = 0.0
    x = x + 0.005 * rng.randn(N)
    at = np.arange(N // HOP + 1) * HOP
    return x.astype(np.float32), glide_f0(at / SR), ~((at >= GAP[0]) & (at < GAP[1]))


def mapped_truth(n_out, rate, ratio=1.0):
    """the contour of an output whose frame t (centred on sample t HOP) plays the input at sample t HOP rate:
    -> (f [T_out] Hz = ratio * glide_f0 there, voiced [T_out])"""
    at = np.arange(n_out // HOP + 1) * HOP * float(rate)
    return ratio * glide_f0(at / SR), ~((at >= GAP[0]) & (at < GAP[1])) & (at < N)


def inner(voiced, margin=4):
    """the voiced frames at least `margin` frames from a voicing edge or an end"""
    v = np.asarray(voiced, bool)
    out = v.copy()
    T = len(v)
    for t in range(T):
        lo, hi = t - margin, t + margin
        if lo < 0 or hi >= T or not v[lo:hi + 1].all():
            out[t] = False
    return out


# ---- the two measures ------------------------------------------------------------------------------------------------------------
def envelope_deviation(y, f_contour, frames):
    """How far the harmonics of y are from the envelope env, in dB rms: frame t (a 400-sample Hann window centred on sample
    t HOP) is projected, by weighted least squares, onto the sinusoids h f_contour[t] <= 2500 Hz; 20 log10(amplitude /
    env(h f)) less its mean over the frame's harmonics; the rms over the harmonics of the inner frames of `frames` (bool [T])."""
    y = np.asarray(y, np.float64)
    W = 400
    win = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(W) + 0.5) / W)
    pad = np.concatenate([np.zeros(W // 2), y, np.zeros(W)])
    j = np.arange(W) - W // 2
    dev = []
    for t in np.nonzero(inner(frames))[0]:
        f = float(f_contour[t])
        hs = np.arange(1, int(2500.0 // f) + 1)
        seg = pad[t * HOP:t * HOP + W]
        arg = 2 * np.pi * np.outer(j, hs * f) / SR
        A = np.concatenate([np.cos(arg), np.sin(arg)], 1) * win[:, None]
        coef = np.linalg.lstsq(A, seg * win, rcond=None)[0]
        amp = np.hypot(coef[:len(hs)], coef[len(hs):])
        db = 20.0 * np.log10(np.maximum(amp, 1e-12) / env(hs * f))
        dev.append(db - db.mean())
    dev = np.concatenate(dev)
    return float(np.sqrt(np.mean(dev ** 2)))


def resample_shift(x, r):
    """the baseline: playback at rate r by linear interpolation -> (y [floor((n - 1) / r) + 1] float32, f_contour, voiced): the
    pitch moves by r, and so does the envelope; scored at the frames mapped by r"""
    x = np.asarray(x, np.float64)
    pos = np.arange(int((len(x) - 1) / r) + 1) * float(r)
    i = np.minimum(pos.astype(np.int64), len(x) - 2)
    fr = pos - i
    y = (1.0 - fr) * x[i] + fr * x[i + 1]
    f, v = mapped_truth(len(y), r, r)
    return y.astype(np.float32), f, v
