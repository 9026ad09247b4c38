"""NumPy float64 replay of the spectral-envelope rule of include/flowtron_hip.h (ft_spectral_envelope), written from the header:
the integers of a frame are formed with np.float32 operations as the header writes them out, everything else is float64 with
numpy's own FFT.  Also the yardsticks the rule is held to that are not the kernel: WORLD's cumulative-sum form of the
smoothing, SPTK's frequency-transform recursion run directly, the project's log-mel cepstra, and the test signal (a pulse
train through three two-pole resonances) with its analytic filter response."""
import math

import numpy as np

F32 = np.float32
F0_CEIL = F32(1000.0)
F0_DEFAULT = F32(500.0)
FLOOR = 1e-20
RESONANCES = ((700.0, 80.0), (1200.0, 100.0), (2600.0, 140.0))           # (centre, bandwidth) Hz


def fft_size(sr, f0_floor=71.0):
    return 2 ** (1 + int(math.floor(math.log2(3.0 * sr / f0_floor + 1.0))))


def frame_integers(f0, sr, n_fft, f0_floor=71.0):
    """the fp32 part of the rule -> dict(f, half, wq, ul, wb, bnd, n_w, fr, wd); f, wq, wb, fr, wd are np.float32"""
    H = n_fft // 2
    f = F32(f0)
    if not (f >= F32(f0_floor) and f <= F0_CEIL):
        f = F0_DEFAULT
    sr15 = F32(1.5 * sr)
    df = F32(sr) / F32(n_fft)
    half = min(int(np.floor(F32(F32(sr15 / f) + F32(0.5)))), H - 1)
    wq = F32(f / df)
    ul = min(2 + int(wq), H)
    wb = F32(F32(F32(F32(2.0) * f) / F32(3.0)) / df)
    bnd = int(wb) + 1
    hw = F32(F32(F32(0.5) * wb) + F32(0.5))
    n_w = min(int(hw), H)
    fr = F32(hw - F32(n_w))
    wd = F32(F32(F32(2.0) * hw) - F32(1.0))
    return dict(f=f, half=half, wq=wq, ul=ul, wb=wb, bnd=bnd, n_w=n_w, fr=fr, wd=wd, df=df, sr15=sr15)


def windowed_frame(x, n, c, g):
    """step 2 -> s [2 half + 1]"""
    i = np.arange(-g["half"], g["half"] + 1)
    idx = np.clip(c + i, 0, n - 1)
    w = 0.5 * np.cos(np.pi * i * float(g["f"]) / float(g["sr15"])) + 0.5
    xw = x[idx].astype(np.float64) * w
    return (xw - w * (xw.sum() / w.sum())) / np.sqrt((w * w).sum())


def dc_correct(P, g):
    """step 4 -> a corrected copy of P"""
    out = P.copy()
    for k in range(g["ul"] - 1):
        pos = F32(g["wq"] - F32(k))
        j = int(pos)
        t = float(pos) - j
        out[k] = P[k] + P[j] + t * (P[j + 1] - P[j])
    return out


def mirror(P, j):
    H = len(P) - 1
    j = np.asarray(j)
    m = np.where(j < 0, -j, np.where(j > H, 2 * H - j, j))
    return P[m]


def smooth_direct(P, g):
    """step 5 without the floor: the whole bins ascending, then the two fractional ends"""
    H = len(P) - 1
    n_w, fr, wd = g["n_w"], float(g["fr"]), float(g["wd"])
    if n_w == 0:
        return P.copy()
    k = np.arange(H + 1)
    acc = np.zeros(H + 1)
    for off in range(-n_w + 1, n_w):                                         # every k at once, each k's bins in ascending order
        acc = acc + mirror(P, k + off)
    acc = acc + fr * (mirror(P, k - n_w) + mirror(P, k + n_w))
    return acc / wd


def smooth_cumsum(P, g):
    """step 5 without the floor in WORLD's form: P mirrored by bnd bins at both ends, the running integral of the piecewise-
    constant spectrum interpolated at the two ends of every interval, their difference over the width (all in bins)"""
    H = len(P) - 1
    bnd, wb = g["bnd"], float(g["wd"])
    j = np.arange(-bnd, H + bnd + 1)
    M = mirror(P, j)
    edges = j - 0.5                                                          # bin j covers [j - 1/2, j + 1/2)
    C = np.concatenate([[0.0], np.cumsum(M)])                                # the integral up to edge j - 1/2, and one behind
    edges = np.concatenate([edges, [j[-1] + 0.5]])
    k = np.arange(H + 1, dtype=np.float64)
    return (np.interp(k + wb / 2, edges, C) - np.interp(k - wb / 2, edges, C)) / wb


def lifter(q, f, sr, q1):
    """the factor of step 6 for quefrency index q >= 1"""
    x = float(f) * q / float(sr)
    return np.sin(np.pi * x) / (np.pi * x) * ((1.0 - 2.0 * q1) + 2.0 * q1 * np.cos(2.0 * np.pi * x))


def frame_envelope(x, n, c, f0, sr, n_fft, f0_floor=71.0, q1=-0.15):
    """one frame -> (env [H + 1], c2 [H + 1] the liftered two-sided cepstrum's q = 0 ..= H)"""
    H = n_fft // 2
    g = frame_integers(f0, sr, n_fft, f0_floor)
    s = windowed_frame(x, n, c, g)
    P = np.abs(np.fft.rfft(s, n_fft)) ** 2
    S = smooth_direct(dc_correct(P, g), g) + FLOOR
    c2 = np.fft.irfft(np.log(S), n_fft)[: H + 1].copy()
    c2[1:] *= lifter(np.arange(1, H + 1), g["f"], sr, float(F32(q1)))
    even = np.concatenate([c2, c2[H - 1:0:-1]])
    return np.exp(np.fft.rfft(even).real), c2


def freqt_direct(c, order, alpha):
    """SPTK's frequency transform of the cepstrum c [m1 + 1] -> [order + 1], the recursion as the header gives it"""
    d = np.zeros(order + 1)
    g = np.zeros(order + 1)
    for i in range(len(c) - 1, -1, -1):
        g[0] = c[i] + alpha * d[0]
        if order >= 1:
            g[1] = (1.0 - alpha * alpha) * d[0] + alpha * d[1]
        for j in range(2, order + 1):
            g[j] = d[j - 1] + alpha * (d[j] - g[j - 1])
        d, g = g, d
    return d.copy()


def one_sided(c2):
    ch = np.array(c2, dtype=np.float64)
    ch[..., 0] *= 0.5
    ch[..., -1] *= 0.5
    return ch


def analyse(x, n, f0, sr, hop, A=None, f0_floor=71.0, q1=-0.15):
    """one utterance x[:n] (x may be longer; nothing behind n is read) -> (env [T, H + 1], c2 [T, H + 1], mc [T, order + 1] or
    None) for its own T = n // hop + 1 frames; A [order + 1, H + 1]: the matrix the device holds (fp32 values) or a float64 one"""
    n_fft = fft_size(sr, f0_floor)
    T, H = n // hop + 1, n_fft // 2
    env, c2 = np.empty((T, H + 1)), np.empty((T, H + 1))
    xs = np.asarray(x)[:n]
    for t in range(T):
        env[t], c2[t] = frame_envelope(xs, n, t * hop, f0[t], sr, n_fft, f0_floor, q1)
    mc = None if A is None else one_sided(c2) @ np.asarray(A, dtype=np.float64).T
    return env, c2, mc


# ---- the test signal and the other yardsticks ---------------------------------------------------------------------------------------

def resonator_coefficients(sr):
    out = []
    for fc, bw in RESONANCES:
        r = math.exp(-math.pi * bw / sr)
        out.append((2.0 * r * math.cos(2.0 * math.pi * fc / sr), -r * r))
    return out


def vowel(f0, sr, n, noise=1e-3, seed=0):
    """a pulse train at f0 Hz (pulses at rounded multiples of the period) through the three two-pole resonances, scaled to a
    peak of 0.5, plus white noise at `noise` of the peak -> float32 [n]"""
    x = np.zeros(n)
    pos = 0.0
    while pos < n:
        x[int(pos)] = 1.0
        pos += sr / f0
    for a1, a2 in resonator_coefficients(sr):
        y = np.zeros(n)
        y1 = y2 = 0.0
        for i in range(n):
            v = x[i] + a1 * y1 + a2 * y2
            y[i] = v
            y2, y1 = y1, v
        x = y
    x *= 0.5 / np.abs(x).max()
    x += noise * 0.5 * np.random.RandomState(seed).standard_normal(n)
    return x.astype(np.float32)


def filter_response_db(freqs, sr):
    """10 log10 |H(f)|^2 of the three resonances in series"""
    z = np.exp(-2j * np.pi * np.asarray(freqs) / sr)
    h = np.ones_like(z)
    for a1, a2 in resonator_coefficients(sr):
        h = h / (1.0 - a1 * z - a2 * z * z)
    return 20.0 * np.log10(np.abs(h))


def mel_filterbank(sr, n_fft, n_mels=80, fmin=0.0, fmax=None):
    """triangular filters on the HTK mel scale, area-normalised (a yardstick of its own: only its cepstra's F0 dependence is used)"""
    fmax = fmax or sr / 2.0
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    imel = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    pts = imel(np.linspace(mel(fmin), mel(fmax), n_mels + 2))
    fr = np.arange(n_fft // 2 + 1) * sr / n_fft
    fb = np.zeros((n_mels, len(fr)))
    for m in range(n_mels):
        lo, ce, hi = pts[m], pts[m + 1], pts[m + 2]
        fb[m] = np.maximum(0.0, np.minimum((fr - lo) / (ce - lo), (hi - fr) / (hi - ce))) * 2.0 / (hi - lo)
    return fb


def logmel_cepstra(x, sr, hop, n_fft=1024, n_mels=80, n_coeffs=13):
    """the project's present recipe on the host: Hann n_fft frames centred on t hop (reflect padding), mel magnitudes, natural
    log clamped at 1e-5, rows 1 .. n_coeffs of the orthonormal DCT-II -> [T, n_coeffs]"""
    x = np.asarray(x, dtype=np.float64)
    xp = np.pad(x, n_fft // 2, mode="reflect")
    T = len(x) // hop + 1
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    fb = mel_filterbank(sr, n_fft, n_mels)
    k = np.arange(1, n_coeffs + 1)[:, None]
    m = np.arange(n_mels)[None, :]
    dct = np.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (m + 0.5) / n_mels)
    out = np.empty((T, n_coeffs))
    for t in range(T):
        mag = np.abs(np.fft.rfft(xp[t * hop: t * hop + n_fft] * w))
        out[t] = dct @ np.log(np.maximum(fb @ mag, 1e-5))
    return out


MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)


def cepstral_distance_db(ca, cb):
    """frame-by-frame MCD of two [T, K] sequences (no c0 among them), dB"""
    return MCD_SCALE * float(np.mean(np.sqrt(((ca - cb) ** 2).sum(axis=1))))
