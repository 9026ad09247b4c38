"""Float64 restatement of the reference's STFT formulas (audio_processing.py:7-75, 172-270) in plain numpy, independent of
flowtron_amd.audio: the one oracle every device result of the audio front end is held to (test_gpu_griffin_lim.py,
test_gpu_stft_pow2.py, test_gpu_vocode_ragged.py), itself held to the real reference's recorded outputs by
test_stft_ref64_cpu.py.  n_fft is always an explicit argument.

    X_t[k] = rfft(w . reflect_pad(y, n_fft / 2)[t hop : t hop + n_fft])[k],   t = 0 .. N // hop
    y[n]   = sum_t w[u - t hop] irfft(M_t e^{i P_t})[u - t hop] / wss[u]  where wss[u] > tiny(float32),   u = n + n_fft / 2
    wss[u] = sum_t w^2[u - t hop]

w is the periodic hann window of win_length samples, zero-padded on both sides to n_fft; numpy's irfft ignores Im of bins 0 and
n_fft / 2 like the reference's pseudo-inverse basis."""
import numpy as np

TINY32 = float(np.finfo(np.float32).tiny)


def hann64(win_length, n_fft):
    w = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    w[lp:lp + win_length] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)
    return w


def stft64(y, n_fft, hop, win_length):
    """complex [B, n_fft/2+1, N // hop + 1]: reflect pad by n_fft/2, hann window, rfft."""
    B, N = y.shape
    w = hann64(win_length, n_fft)
    yp = np.pad(np.asarray(y, np.float64), ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    idx = np.arange(N // hop + 1)[:, None] * hop + np.arange(n_fft)[None, :]
    return np.fft.rfft(yp[:, idx] * w, axis=2).transpose(0, 2, 1)


def wss64(T, n_fft, hop, win_length):
    """The window's sum-square envelope over the n_fft + hop (T - 1) untrimmed samples of T frames."""
    w2 = hann64(win_length, n_fft) ** 2
    out = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        out[t * hop:t * hop + n_fft] += w2
    return out


def istft64(M, P, n_fft, hop, win_length):
    """(y [B, hop (T-1)], wss over the same samples): windowed irfft of every frame, overlap-add in ascending t, division by the
    envelope where it is > tiny(float32), n_fft/2 samples cut at both ends."""
    B, _, T = M.shape
    w = hann64(win_length, n_fft)
    fr = np.fft.irfft(np.asarray(M, np.float64) * np.exp(1j * np.asarray(P, np.float64)), n=n_fft, axis=1) * w[None, :, None]
    n = n_fft + hop * (T - 1)
    out = np.zeros((B, n))
    for t in range(T):
        out[:, t * hop:t * hop + n_fft] += fr[:, :, t]
    wss = wss64(T, n_fft, hop, win_length)
    nz = wss > TINY32
    out[:, nz] /= wss[nz]
    h = n_fft // 2
    return out[:, h:n - h], wss[h:n - h]


def griffin_lim64(M, angles, n_iters, n_fft, hop, win_length):
    y = istft64(M, angles, n_fft, hop, win_length)[0]
    for _ in range(n_iters):
        y = istft64(M, np.angle(stft64(y, n_fft, hop, win_length)), n_fft, hop, win_length)[0]
    return y


def start_angles(shape, seed=0):
    """The starting phase griffin_lim draws under np.random.seed(seed), rounded to float32 as it is on the device."""
    np.random.seed(seed)
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
