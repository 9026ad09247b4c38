"""Host restatements of the two vocoding kernels of csrc/vocode.hip, independent of flowtron_amd.audio:

nnls(..., dtype): the arithmetic rule of ft_mel_nnls (include/flowtron_hip.h) operation by operation in `dtype`; numpy rounds
every float32 ufunc once and fuses nothing, so `nnls32` gives the kernel's bits and `nnls64` is the same iteration in float64.
fast_griffin_lim64: Griffin-Lim with momentum (Perraudin et al. 2013) from stft_ref64's stft64 / istft64, with t_1 = c_1."""
import numpy as np

from stft_ref64 import istft64, stft64

PARTS = 16                                        # partial sums of the start's mean
FLOOR32, TINY32_M = np.float32(1e-3), np.float32(1e-30)


def tables(W):
    """Dense [n_mel, n_bins] filterbank -> (bin0, ptr, w, band [n_bins, 2], weight [n_bins, 2]): every band one run of
    consecutive bins from its first to its last non-zero; per bin the bands whose run holds it, lower first, -1 where none."""
    W = np.asarray(W, np.float32)
    bin0, ptr, w = [], [0], []
    for row in W:
        nz = np.nonzero(row)[0]
        if len(nz) == 0:
            bin0.append(0)
            ptr.append(ptr[-1])
            continue
        bin0.append(int(nz[0]))
        w.extend(row[nz[0]:nz[-1] + 1].tolist())
        ptr.append(len(w))
    bin0, ptr, w = np.asarray(bin0, np.int32), np.asarray(ptr, np.int32), np.asarray(w, np.float32)
    band = np.full((W.shape[1], 2), -1, np.int32)
    weight = np.zeros((W.shape[1], 2), np.float32)
    for j in range(W.shape[0]):
        for i in range(ptr[j + 1] - ptr[j]):
            k = bin0[j] + i
            c = int((band[k] >= 0).sum())
            assert c < 2, "bin %d lies in more than two bands" % k
            band[k, c], weight[k, c] = j, w[ptr[j] + i]
    return bin0, ptr, w, band, weight


def _band(x, bin0, ptr, w, dtype):
    """[n_bins, F] -> [n_mel, F]: every band adds its bins in ascending order, from 0."""
    lens = np.diff(ptr)
    out = np.zeros((len(bin0), x.shape[1]), dtype)
    for i in range(int(lens.max())):
        on = np.nonzero(lens > i)[0]
        out[on] = out[on] + w[ptr[on] + i].astype(dtype)[:, None] * x[bin0[on] + i]
    return out


def _bin(y, band, weight, dtype):
    """[n_mel, F] -> [n_bins, F]: the lower band's product, then the upper band's added; 0 on uncovered bins."""
    out = np.zeros((len(band), y.shape[1]), dtype)
    one = np.nonzero(band[:, 0] >= 0)[0]
    out[one] = weight[one, 0].astype(dtype)[:, None] * y[band[one, 0]]
    two = np.nonzero(band[:, 1] >= 0)[0]
    out[two] = out[two] + weight[two, 1].astype(dtype)[:, None] * y[band[two, 1]]
    return out


def nnls(W, s, m0, n_iters, dtype, history=False):
    """s [n_mel, F] linear mel, m0 [n_bins, F] start estimate (frames are columns) -> m [n_bins, F] in `dtype`; history=True
    returns the list of the n_iters + 1 iterates instead."""
    bin0, ptr, w, band, weight = tables(W)
    s, m0 = np.asarray(s, np.float32).astype(dtype), np.asarray(m0, np.float32).astype(dtype)
    nb, F = m0.shape
    covered = band[:, 0] >= 0
    p = np.zeros((PARTS, F), dtype)
    for q in range(0, nb, PARTS):
        rows = m0[q:q + PARTS]
        p[:len(rows)] = p[:len(rows)] + rows
    total = np.zeros(F, dtype)
    for l in range(PARTS):
        total = total + p[l]
    low = dtype(FLOOR32) * (total / dtype(nb))
    m = np.where(covered[:, None], np.where(m0 < low[None, :], low[None, :], m0), dtype(0)).astype(dtype)
    q = _bin(s, band, weight, dtype)
    out = [m.copy()]
    for _ in range(n_iters):
        d = _bin(_band(m, bin0, ptr, w, dtype), band, weight, dtype)
        pos = d > 0
        new = np.zeros_like(m)
        new[pos] = (m[pos] * q[pos]) / d[pos]
        new[new < dtype(TINY32_M)] = 0
        new[~covered] = 0
        m = new
        if history:
            out.append(m.copy())
    assert m.dtype == dtype
    return out if history else m


def nnls32(W, s, m0, n_iters, history=False):
    return nnls(W, s, m0, n_iters, np.float32, history)


def nnls64(W, s, m0, n_iters, history=False):
    return nnls(W, s, m0, n_iters, np.float64, history)


def pinv_relu(W, s):
    """Today's estimate in float64: relu(pinv(W) s)."""
    return np.maximum(np.linalg.pinv(np.asarray(W, np.float64)) @ np.asarray(s, np.float64), 0)


def residual(W, m, s):
    """||W m - s|| per frame, float64."""
    return np.linalg.norm(np.asarray(W, np.float64) @ np.asarray(m, np.float64) - np.asarray(s, np.float64), axis=0)


def fast_griffin_lim64(M, angles, n_iters, n_fft, hop, win_length, momentum):
    """griffin_lim64 with the momentum step: c_n = stft(y_n), t_1 = c_1, t_n = c_n + momentum (c_n - c_{n-1}),
    y_{n+1} = istft(M, angle(t_n))."""
    y = istft64(M, angles, n_fft, hop, win_length)[0]
    prev = None
    for _ in range(n_iters):
        c = stft64(y, n_fft, hop, win_length)
        t = c if prev is None else c + momentum * (c - prev)
        prev = c
        y = istft64(M, np.angle(t), n_fft, hop, win_length)[0]
    return y


def spectral_convergence(y, M, n_fft, hop, win_length):
    M = np.asarray(M, np.float64)
    return float(np.linalg.norm(np.abs(stft64(y, n_fft, hop, win_length)) - M) / np.linalg.norm(M))
