"""Float64 restatement of the reference's STFT formulas (audio_processing.py:7-75, 172-270) in plain numpy, independent of
flowtron_amd.audio: the one oracle every device result of the audio front end is held to (test_gpu_griffin_lim.py,
test_gpu_stft_pow2.py, test_gpu_vocode_ragged.py, test_gpu_stft_front_end_f64.py, test_gpu_istft_f64.py), itself held to the real reference's recorded outputs by
test_stft_ref64_cpu.py.  n_fft is always an explicit argument.

    X_t[k] = rfft(w . reflect_pad(y, n_fft / 2)[t hop : t hop + n_fft])[k],   t = 0 .. N // hop
    y[n]   = sum_t w[u - t hop] irfft(M_t e^{i P_t})[u - t hop] / wss[u]  where wss[u] > tiny(float32),   u = n + n_fft / 2
    wss[u] = sum_t w^2[u - t hop]

w is the periodic hann window of win_length samples, zero-padded on both sides to n_fft; numpy's irfft ignores Im of bins 0 and
n_fft / 2 like the reference's pseudo-inverse basis.

The second half is the mel front end's: the float64 log-mel, the kernels' single-fold padding rule, the derived per-element
bound on a log-mel (logmel_judge), two hand-made CSR filterbanks that reach what no Slaney filterbank does, and six deliberately
wrong references the bound must keep out.

The last part is the inverse's (test_gpu_istft_f64.py, test_istft_ref64_cpu.py): the derived per-sample bound of an fp32 inverse
(inverse_bound + overlap_add_bound = istft_bound), the reference of a ragged batch, and nine deliberately wrong inverses
(ISTFT_MUTATIONS)."""
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


def wss64(T, n_fft, hop, win_length, window=None):
    """The window's sum-square envelope over the n_fft + hop (T - 1) untrimmed samples of T frames.  window: the n_fft taps to
    use in place of hann64 (the module's float32 window, widened)."""
    w2 = (hann64(win_length, n_fft) if window is None else np.asarray(window, np.float64)) ** 2
    out = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        out[t * hop:t * hop + n_fft] += w2
    return out


def istft64(M, P, n_fft, hop, win_length, window=None):
    """(y [B, hop (T-1)], wss over the same samples): windowed irfft of every frame, overlap-add in ascending t, division by the
    envelope where it is > tiny(float32), n_fft/2 samples cut at both ends.  window: as wss64."""
    B, _, T = M.shape
    w = hann64(win_length, n_fft) if window is None else np.asarray(window, np.float64)
    fr = np.fft.irfft(np.asarray(M, np.float64) * np.exp(1j * np.asarray(P, np.float64)), n=n_fft, axis=1) * w[None, :, None]
    n = n_fft + hop * (T - 1)
    out = np.zeros((B, n))
    for t in range(T):
        out[:, t * hop:t * hop + n_fft] += fr[:, :, t]
    wss = wss64(T, n_fft, hop, win_length, window)
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


# ---- the inverse: the derived per-sample bound, the ragged reference, deliberately wrong inverses -------------------------------
EPS32 = 2.0 ** -23                                       # fp32 machine epsilon = 2 U32


def clamp_frames(n, T):
    """The inverse kernels' own rule for a ragged frame count: min(max(n, 1), T)."""
    return min(max(int(n), 1), T)


def _window64(n_fft, win_length, window):
    return hann64(win_length, n_fft) if window is None else np.asarray(window, np.float64)


def _ola64(fr, hop):
    """overlap-add [B, n_fft, T] -> [B, n_fft + hop (T-1)], ascending t."""
    B, n_fft, T = fr.shape
    out = np.zeros((B, n_fft + hop * (T - 1)))
    for t in range(T):
        out[:, t * hop:t * hop + n_fft] += fr[:, :, t]
    return out


def _each_utterance(fn, M, P, hop, n_frames):
    """[B, hop (T-1)]: row b holds fn(M[b:b+1, :, :n], P[b:b+1, :, :n])[0] in its samples [0, hop (n - 1)), n =
    clamp_frames(n_frames[b], T), and zeros behind -- what a ragged launch must write.  One frame gives a row of zeros.  The
    frames behind n are never touched (they may hold NaN)."""
    B, _, T = M.shape
    assert len(n_frames) == B
    out = np.zeros((B, hop * (T - 1)))
    for b in range(B):
        n = clamp_frames(n_frames[b], T)
        if n >= 2:
            out[b, :hop * (n - 1)] = fn(M[b:b + 1, :, :n], P[b:b + 1, :, :n])[0]
    return out


def istft64_ragged(M, P, n_fft, hop, win_length, n_frames, window=None):
    """y [B, hop (T-1)] of a ragged batch: every utterance by istft64 on its own frames alone, zeros behind."""
    return _each_utterance(lambda m, p: istft64(m, p, n_fft, hop, win_length, window)[0], M, P, hop, n_frames)


def inverse_bound(M, n_fft, hop, win_length, n_frames=None, window=None):
    """The FFT term of the per-sample bound on |fp32 inverse - float64 restatement|, [B, hop (T-1)].  One output x[m] of a
    frame's fp32 irfft is built from the spectrum through log2(n_fft) levels of butterflies (the radix passes and the split
    step); every level rounds each partial sum once, and no partial sum exceeds A_t = sum over the full Hermitian spectrum of
    |X_t[k]| / n_fft (the largest value any sample of that frame can take; bins 0 and n_fft/2 count once).  So |error of
    x[m]| <= c eps log2(n_fft) A_t, where c = 4 covers the complex twiddle products (|relative error| <= sqrt(5) eps) and the
    sincosf of X = M e^{i phase} (<= 2 ulp).  Windowed, added over the frames that cover a sample and divided by the envelope
    where the kernels divide, with a factor 2 of margin:  bound[n] = 8 eps log2(n_fft) sum_t w A_t / wss[u].  It is a worst
    case: FFT rounding errors add up like a random walk, so the observed error is far below it (reported by the tests).

    What the window product, the ordered overlap-add, the envelope sum and the division add on top is overlap_add_bound; the
    two together are istft_bound.  (test_gpu_griffin_lim.py, whose hops give at most 8 overlapping frames, keeps its own 8 eps
    |y| for them.)  n_frames [B]: a ragged batch, every utterance bounded from its own clamp_frames(n_frames[b], T) frames,
    zero behind its end, where a launch must write exact zeros.  window: as wss64."""
    if n_frames is not None:
        return _each_utterance(lambda m, p: inverse_bound(m, n_fft, hop, win_length, None, window), M, M, hop, n_frames)
    B, _, T = M.shape
    M = np.asarray(M, np.float64)
    H = n_fft // 2
    A = (2 * M.sum(axis=1) - M[:, 0] - M[:, H]) / n_fft                  # [B, T]
    w = _window64(n_fft, win_length, window)
    env = _ola64(np.abs(w)[None, :, None] * A[:, None, :], hop)
    wss = wss64(T, n_fft, hop, win_length, window)
    nz = wss > TINY32
    env[:, nz] /= wss[nz]
    return 8 * EPS32 * np.log2(n_fft) * env[:, H:env.shape[1] - H]


def overlap_add_bound(M, P, n_fft, hop, win_length, n_frames=None, window=None):
    """What an fp32 inverse loses after its FFTs, per sample [B, hop (T-1)], derived (u = 2^-24, gamma_k = k u / (1 - k u)):

      * acc = fl(sum_t fl(w x_t)) over the K frames whose window tap on the sample is not zero (a zero tap adds an exact
        zero), in any fixed order: each product rounds once and the sum K - 1 times, so |acc' - acc| <= gamma_K S with
        S = sum_t |w x_t| (Higham, Accuracy and Stability, 4.4);
      * wss' = fl(sum_t fl(w^2)): K products and K - 1 additions of non-negative terms, wss' = wss (1 + theta),
        |theta| <= gamma_K;
      * y' = fl(acc' / wss') rounds once more.
    So |y' - y| <= (gamma_K S / wss + gamma_{K+1} |y|) / (1 - gamma_{K+1}), and gamma_K S where the envelope is not divided
    by.  At hop 256 K is 4; at hop 1 it is up to n_fft, where "a few eps" no longer says it.  x_t here is the float64 frame:
    the fp32 frame's own error times gamma_K is of second order and inside the factor 2 of inverse_bound."""
    if n_frames is not None:
        return _each_utterance(lambda m, p: overlap_add_bound(m, p, n_fft, hop, win_length, None, window), M, P, hop, n_frames)
    B, _, T = M.shape
    w = _window64(n_fft, win_length, window)
    fr = _iframes64(M, P, n_fft, w)
    S = _ola64(np.abs(fr), hop)
    K = _ola64(np.broadcast_to((w != 0).astype(np.float64)[None, :, None], (1, n_fft, T)), hop)[0]
    wss = wss64(T, n_fft, hop, win_length, window)
    nz = wss > TINY32
    gK, gK1 = K * U32 / (1 - K * U32), (K + 1) * U32 / (1 - (K + 1) * U32)
    y = _ola64(fr, hop)
    y[:, nz] /= wss[nz]
    out = gK * S
    out[:, nz] = ((gK * S)[:, nz] / wss[nz] + gK1[nz] * np.abs(y[:, nz])) / (1 - gK1[nz])
    H = n_fft // 2
    return out[:, H:out.shape[1] - H]


def istft_bound(M, P, n_fft, hop, win_length, n_frames=None, window=None):
    """The whole per-sample bound of an fp32 inverse against istft64 / istft64_ragged on the same window: FFT term plus
    overlap-add term.  Nothing in it was fitted to a kernel (test_istft_ref64_cpu.py holds an fp32 inverse written with
    torch.fft to it)."""
    return (inverse_bound(M, n_fft, hop, win_length, n_frames, window)
            + overlap_add_bound(M, P, n_fft, hop, win_length, n_frames, window))


def istft_ratio(got, ref, bound):
    """|got - ref| / bound per sample; 0 where both vanish (a sample that must be exact and is), inf where only the bound does,
    and inf for a NaN."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1.0))
    r = np.where((err > 0) & ~(bound > 0), np.inf, r)
    return np.where(np.isnan(err), np.inf, r)


def _iframes64(M, P, n_fft, w, keep_im=False):
    """The windowed frames [B, n_fft, T].  keep_im: Im X[0] = b and Im X[n_fft/2] = d are not dropped before the inverse
    split step Z[0] = (X[0] + conj X[H]) + i (X[0] - conj X[H]), which then carries -(b + d) + i (b - d) more: every even
    sample of the frame moves by -(b + d) / n_fft and every odd one by (b - d) / n_fft."""
    X = np.asarray(M, np.float64) * np.exp(1j * np.asarray(P, np.float64))
    fr = np.fft.irfft(X, n=n_fft, axis=1)
    if keep_im:
        b, d = X[:, 0].imag[:, None, :], X[:, -1].imag[:, None, :]
        even = (np.arange(n_fft) % 2 == 0)[None, :, None]
        fr = fr + np.where(even, -(b + d), b - d) / n_fft
    return fr * w[None, :, None]


def _finish64(acc, wss, n_fft, divide=None, start=None):
    """Divide acc where `divide` (default wss > tiny(float32)) and cut to the hop (T-1) samples from `start` (n_fft/2) on."""
    out = acc.copy()
    nz = wss > TINY32 if divide is None else divide
    out[:, nz] /= wss[nz]
    s = n_fft // 2 if start is None else start
    return out[:, s:s + out.shape[1] - n_fft]


def default_span(n_fft, hop):
    """The output samples a workgroup owns: 16 hop in istft_r8_k (n_fft 1024, hop <= 256), 4 096 in istft_pow2_k."""
    return 16 * hop if n_fft == 1024 and hop <= 256 else 4096


def _wrong_inverse(fn):
    """fn(M, P, n_fft, hop, w, win_length, span) -> y, made into (M, P, n_fft, hop, win_length, window=None, n_frames=None,
    span=None): istft64's arguments plus the ragged counts and the workgroup span."""
    def run(M, P, n_fft, hop, win_length, window=None, n_frames=None, span=None):
        sp = default_span(n_fft, hop) if span is None else span

        def one(m, p):
            return fn(m, p, n_fft, hop, _window64(n_fft, win_length, window), win_length, sp)
        return one(M, P) if n_frames is None else _each_utterance(one, M, P, hop, n_frames)
    run.__doc__ = fn.__doc__
    return run


@_wrong_inverse
def imut_drop_first_halo(M, P, n_fft, hop, w, win_length, span):
    """Every workgroup span behind the first adds its frames from t_lo + 1 on: the first halo frame, the earliest that
    covers the span's first sample, is missing from that span's sums (the envelope, summed apart, is whole)."""
    T = M.shape[2]
    fr = _iframes64(M, P, n_fft, w)
    acc = _ola64(fr, hop)
    H, n_out = n_fft // 2, hop * (T - 1)
    for n0 in range(span, n_out, span):
        u0, u1 = n0 + H, min(n0 + span, n_out) + H
        t_lo = 0 if u0 - (n_fft - 1) <= 0 else -(-(u0 - (n_fft - 1)) // hop)
        if 0 < t_lo < T:
            lo, hi = max(u0, t_lo * hop), min(u1, t_lo * hop + n_fft)
            acc[:, lo:hi] -= fr[:, lo - t_lo * hop:hi - t_lo * hop, t_lo]
    return _finish64(acc, wss64(T, n_fft, hop, win_length, w), n_fft)


@_wrong_inverse
def imut_wss_short(M, P, n_fft, hop, w, win_length, span):
    """The envelope of a sample leaves out its last covering frame min(T - 1, u / hop)."""
    T = M.shape[2]
    wss = wss64(T, n_fft, hop, win_length, w)
    u = np.arange(wss.size)
    wss = np.maximum(wss - w[u - np.minimum(T - 1, u // hop) * hop] ** 2, 0.0)
    return _finish64(_ola64(_iframes64(M, P, n_fft, w), hop), wss, n_fft)


def imut_wss_batch_T(M, P, n_fft, hop, win_length, window=None, n_frames=None, span=None):
    """Ragged only: the last covering frame and the envelope of a sample come from the batch's T, not the utterance's own
    count -- the frames behind the utterance (read as silence here) are added and their window squares counted."""
    if n_frames is None:
        raise ValueError("wss_batch_T is a defect of the ragged form: n_frames is required")
    B, _, T = M.shape
    out = np.zeros((B, hop * (T - 1)))
    for b in range(B):
        n = clamp_frames(n_frames[b], T)
        m, p = np.zeros((1,) + M.shape[1:]), np.zeros((1,) + M.shape[1:])
        m[:, :, :n], p[:, :, :n] = M[b:b + 1, :, :n], P[b:b + 1, :, :n]
        out[b, :hop * (n - 1)] = istft64(m, p, n_fft, hop, win_length, window)[0][0, :hop * (n - 1)]
    return out


@_wrong_inverse
def imut_trim_shift(M, P, n_fft, hop, w, win_length, span):
    """The output starts at untrimmed sample n_fft / 2 + 1."""
    T = M.shape[2]
    return _finish64(_ola64(_iframes64(M, P, n_fft, w), hop), wss64(T, n_fft, hop, win_length, w), n_fft, start=n_fft // 2 + 1)


@_wrong_inverse
def imut_divide_always(M, P, n_fft, hop, w, win_length, span):
    """Division everywhere, also where wss <= tiny(float32); 0 / 0 is guarded to 1e30."""
    T = M.shape[2]
    wss = wss64(T, n_fft, hop, win_length, w)
    acc = _ola64(_iframes64(M, P, n_fft, w), hop)
    acc[:, wss == 0] = 1e30
    return _finish64(acc, wss, n_fft, divide=wss > 0)


@_wrong_inverse
def imut_divide_late(M, P, n_fft, hop, w, win_length, span):
    """No division where wss < 1e-6."""
    T = M.shape[2]
    wss = wss64(T, n_fft, hop, win_length, w)
    return _finish64(_ola64(_iframes64(M, P, n_fft, w), hop), wss, n_fft, divide=wss >= 1e-6)


@_wrong_inverse
def imut_symmetric_hann(M, P, n_fft, hop, w, win_length, span):
    """Symmetric instead of periodic hann."""
    T = M.shape[2]
    w = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    w[lp:lp + win_length] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / (win_length - 1))
    return _finish64(_ola64(_iframes64(M, P, n_fft, w), hop), wss64(T, n_fft, hop, win_length, w), n_fft)


@_wrong_inverse
def imut_window_uncentred(M, P, n_fft, hop, w, win_length, span):
    """win_length < n_fft: the window's taps start at 0 instead of (n_fft - win_length) // 2."""
    T = M.shape[2]
    w = np.roll(w, -((n_fft - win_length) // 2))
    return _finish64(_ola64(_iframes64(M, P, n_fft, w), hop), wss64(T, n_fft, hop, win_length, w), n_fft)


@_wrong_inverse
def imut_keep_im_dc_nyquist(M, P, n_fft, hop, w, win_length, span):
    """The imaginary parts of bins 0 and n_fft / 2 contribute (_iframes64)."""
    T = M.shape[2]
    return _finish64(_ola64(_iframes64(M, P, n_fft, w, keep_im=True), hop), wss64(T, n_fft, hop, win_length, w), n_fft)


ISTFT_MUTATIONS = {"drop_first_halo": imut_drop_first_halo, "wss_short": imut_wss_short, "wss_batch_T": imut_wss_batch_T,
                   "trim_shift": imut_trim_shift, "divide_always": imut_divide_always, "divide_late": imut_divide_late,
                   "symmetric_hann": imut_symmetric_hann, "window_uncentred": imut_window_uncentred,
                   "keep_im_dc_nyquist": imut_keep_im_dc_nyquist}
