"""Float64 restatement of the reference's STFT formulas (audio_processing.py:7-75, 172-270) in plain numpy, independent of
flowtron_amd.audio: the one oracle every device result of the audio front end is held to (test_gpu_griffin_lim.py,
test_gpu_stft_pow2.py, test_gpu_vocode_ragged.py, test_gpu_stft_front_end_f64.py), itself held to the real reference's recorded outputs by
test_stft_ref64_cpu.py.  n_fft is always an explicit argument.

    X_t[k] = rfft(w . reflect_pad(y, n_fft / 2)[t hop : t hop + n_fft])[k],   t = 0 .. N // hop
    y[n]   = sum_t w[u - t hop] irfft(M_t e^{i P_t})[u - t hop] / wss[u]  where wss[u] > tiny(float32),   u = n + n_fft / 2
    wss[u] = sum_t w^2[u - t hop]

w is the periodic hann window of win_length samples, zero-padded on both sides to n_fft; numpy's irfft ignores Im of bins 0 and
n_fft / 2 like the reference's pseudo-inverse basis.

The second half is the mel front end's: the float64 log-mel, the kernels' single-fold padding rule, the derived per-element
bound on a log-mel (logmel_judge), two hand-made CSR filterbanks that reach what no Slaney filterbank does, and six deliberately
wrong references the bound must keep out."""
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


# ---- the mel front end: float64 log-mel, the derived per-element bound, hand-made filterbanks, wrong references ---------------
# MAG_BOUND and PHASE_BOUND are the bounds test_gpu_stft_pow2.py holds every power-of-two transform to (the ~eps log2 N estimate of
# an fp32 FFT; n_fft 1024 is inside that file's grid): per-frame magnitude relative L2 and phase where |X| > 1e-3 max|X|.
MAG_BOUND, PHASE_BOUND = 1e-6, 1e-4
U32 = 2.0 ** -24                                         # fp32 unit roundoff
FLOOR = 1e-5                                             # dynamic_range_compression's clip_val (audio_processing.py:81-82)


def mel64(y, n_fft, hop, win, fb):
    """log(max(fb . |stft64(y)|, 1e-5)) [B, n_mel, T]; fb [n_mel, n_fft/2+1]: the float32 weights the kernel sees, widened."""
    return np.log(np.maximum(np.einsum("mk,bkt->bmt", np.asarray(fb, np.float64), np.abs(stft64(y, n_fft, hop, win))), FLOOR))


def csr_dense64(bin0, ptr, w, n_bins):
    """The dense [n_mel, n_bins] float64 matrix of a CSR filterbank: band m holds w[ptr[m] : ptr[m+1]] from bin bin0[m] on."""
    n_mel = len(bin0)
    fb = np.zeros((n_mel, n_bins))
    for m in range(n_mel):
        n = int(ptr[m + 1] - ptr[m])
        assert int(bin0[m]) + n <= n_bins, (m, int(bin0[m]), n)
        fb[m, int(bin0[m]):int(bin0[m]) + n] = np.asarray(w[int(ptr[m]):int(ptr[m + 1])], np.float64)
    return fb


def stft64_single_fold(y, n_fft, hop, win_length):
    """The spectrum under the kernels' own padding rule (stft_r8.hip: n < 0 -> -n, then n >= N -> 2 (N - 1) - n, zero where the
    index still falls outside [0, N)): one reflection at each end.  For N > n_fft / 2 this is stft64; for a shorter signal,
    which numpy's reflect padding would fold several times, it is what a ragged launch computes."""
    B, N = y.shape
    w = hann64(win_length, n_fft)
    n = np.arange(N // hop + 1)[:, None] * hop + np.arange(n_fft)[None, :] - n_fft // 2
    n = np.where(n < 0, -n, n)
    n = np.where(n >= N, 2 * (N - 1) - n, n)
    inside = (n >= 0) & (n < N)
    fr = np.where(inside[None], np.asarray(y, np.float64)[:, np.clip(n, 0, N - 1)], 0.0)
    return np.fft.rfft(fr * w, axis=2).transpose(0, 2, 1)


def frame_rel_l2(mag, absX64):
    """[B, T]: relative L2 error of every frame's magnitudes alone (a silent frame of the reference counts by its absolute
    error, which must then be zero)."""
    d = np.linalg.norm(np.asarray(mag, np.float64) - absX64, axis=1)
    n = np.linalg.norm(absX64, axis=1)
    return np.where(n > 0, d / np.where(n > 0, n, 1.0), d)


def phase_mask(absX64):
    """The bins whose phase is judged: |X| > 1e-3 of the largest magnitude of the tensor (test_gpu_stft_pow2.py)."""
    return absX64 > 1e-3 * absX64.max()


def frame_phase_err(phase, X64):
    """[B, T]: the largest wrapped phase error of every frame over its masked bins (0 where a frame has none)."""
    d = np.abs(np.remainder(np.asarray(phase, np.float64) - np.angle(X64) + np.pi, 2 * np.pi) - np.pi)
    return np.where(phase_mask(np.abs(X64)), d, 0.0).max(axis=1)


def logmel_judge(got, absX64, fb, center=None):
    """Per-element ratio error / allowance of a log-mel `got` [B, n_mel, T] against s = fb . |X| in float64; <= 1 passes.

    A kernel forms s' = fl(sum_k w_k m_k) from its own fp32 magnitudes m and logf(max(s', 1e-5)).  With the per-frame
    magnitude bound ||m_t - |X_t|||_2 <= MAG_BOUND ||X_t||_2 and Cauchy-Schwarz, |sum_k w_k (m_k - |X_k|)| <=
    ||fb_m||_2 MAG_BOUND ||X_t||_2; the n_m products and n_m - 1 additions of non-negative terms, in any order, lose at most
    (n_m + 2) 2^-24 s to first order.  So s' lies within delta = ||fb_m||_2 MAG_BOUND ||X_t||_2 + (n_m + 2) 2^-24 s of s, the
    result within [log max(s - delta, 1e-5), log max(s + delta, 1e-5)], and logf adds 4 x 2^-24 max(1, |log|) at each end.
    The ratio is the distance from `center` (default log max(s, 1e-5)) over the half-width of the side it falls on; with
    `center` a device result and `got` a wrong reference it says how far that reference is from the device, in bounds."""
    fb = np.asarray(fb, np.float64)
    s = np.einsum("mk,bkt->bmt", fb, absX64)
    n_m = (fb != 0).sum(axis=1)
    delta = (np.linalg.norm(fb, axis=1)[None, :, None] * MAG_BOUND * np.linalg.norm(absX64, axis=1)[:, None, :]
             + (n_m + 2)[None, :, None] * U32 * s)
    mid = np.log(np.maximum(s, FLOOR))
    lo = np.log(np.maximum(s - delta, FLOOR))
    hi = np.log(np.maximum(s + delta, FLOOR))
    lo = lo - 4 * U32 * np.maximum(1.0, np.abs(lo))
    hi = hi + 4 * U32 * np.maximum(1.0, np.abs(hi))
    c = mid if center is None else np.asarray(center, np.float64)
    d = np.asarray(got, np.float64) - c
    return np.where(d >= 0, d / (hi - mid), -d / (mid - lo))


HANDMADE_WIDTHS = {"WIDE": (17,), "NARROW": (1, 7, 8, 9, 16, 17)}
HANDMADE_EMPTY, HANDMADE_BIN0, HANDMADE_LAST = 125, 126, 127         # the three special bands


def handmade_csr(kind, n_bins):
    """(bin0 int32 [128], ptr int32 [129], w float32 [nnz]): 128 bands over n_bins = 513 bins, or the scaled twin at 257.
    Bands 0 .. 124 start at bin m (n_bins - 17) // 124 (4 m at 513) and their widths cycle through HANDMADE_WIDTHS[kind], so a
    17-bin band 124 ends on the last bin; band 125 is empty, band 126 holds bin 0 alone and band 127 the last bin alone.
    Positive weights from a fixed seed.  WIDE: 125 x 17 + 2 = 2 127 weights, more than the 2 048 the kernels stage in LDS;
    NARROW: 1 203, staged, with widths on both sides of the eight-at-a-time weight loop."""
    widths = HANDMADE_WIDTHS[kind]
    rs = np.random.RandomState(513 + len(widths))
    bin0, ptr, w = [], [0], []
    for m in range(125):
        n = widths[m % len(widths)]
        bin0.append(m * (n_bins - 17) // 124)
        w.extend(rs.uniform(0.05, 1.0, n).tolist())
        ptr.append(len(w))
    for first, n in ((0, 0), (0, 1), (n_bins - 1, 1)):
        bin0.append(first)
        w.extend(rs.uniform(0.05, 1.0, n).tolist())
        ptr.append(len(w))
    return np.asarray(bin0, np.int32), np.asarray(ptr, np.int32), np.asarray(w, np.float32)


# ---- wrong references: each takes (y, (n_fft, hop, win), fb) and returns the log-mel of a deliberately wrong statement -----------
def _frames64(y, n_fft, hop, pad_mode="reflect", offset=0):
    B, N = y.shape
    yp = np.pad(np.asarray(y, np.float64), ((0, 0), (n_fft // 2, n_fft // 2 + offset)), mode=pad_mode)
    return yp[:, np.arange(N // hop + 1)[:, None] * hop + np.arange(n_fft)[None, :] + offset]


def _logmel(absX, fb, floor=FLOOR):
    return np.log(np.maximum(np.einsum("mk,bkt->bmt", np.asarray(fb, np.float64), absX), floor))


def _abs_rfft(fr, w):
    return np.abs(np.fft.rfft(fr * w, axis=2).transpose(0, 2, 1))


def mut_edge_reflect(y, settings, fb):
    """Reflection that repeats the edge sample (n = -n - 1)."""
    n_fft, hop, win = settings
    return _logmel(_abs_rfft(_frames64(y, n_fft, hop, "symmetric"), hann64(win, n_fft)), fb)


def mut_drop_last_bin(y, settings, fb):
    """Every band's last bin dropped."""
    fb = np.array(fb, np.float64)
    for row in fb:
        nz = np.nonzero(row)[0]
        if len(nz):
            row[nz[-1]] = 0.0
    return _logmel(np.abs(stft64(y, *settings)), fb)


def mut_bin0_shift(y, settings, fb):
    """Every band's first bin shifted up by one (a weight that would pass the last bin is dropped)."""
    fb = np.asarray(fb, np.float64)
    sh = np.zeros_like(fb)
    sh[:, 1:] = fb[:, :-1]
    return _logmel(np.abs(stft64(y, *settings)), sh)


def mut_floor(y, settings, fb):
    """Floor 1e-6 instead of 1e-5."""
    return _logmel(np.abs(stft64(y, *settings)), fb, 1e-6)


def mut_symmetric_hann(y, settings, fb):
    """Symmetric instead of periodic hann."""
    n_fft, hop, win = settings
    w = np.zeros(n_fft)
    lp = (n_fft - win) // 2
    w[lp:lp + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / (win - 1))
    return _logmel(_abs_rfft(_frames64(y, n_fft, hop), w), fb)


def mut_frame_offset(y, settings, fb):
    """Frame t taken at t hop + 1."""
    n_fft, hop, win = settings
    return _logmel(_abs_rfft(_frames64(y, n_fft, hop, offset=1), hann64(win, n_fft)), fb)


MUTATIONS = {"edge_reflect": mut_edge_reflect, "drop_last_bin": mut_drop_last_bin, "bin0_shift": mut_bin0_shift,
             "floor_1e-6": mut_floor, "symmetric_hann": mut_symmetric_hann, "frame_offset": mut_frame_offset}
