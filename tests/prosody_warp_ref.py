"""NumPy replay of the time-map rules (include/flowtron_hip.h, a pace that varies within the utterance; csrc/prosody.hip), written
from the header, on top of tests/prosody_ref.py (per[], the analysis marks, the source choice, half and synth() are that
file's), and the transfer signal the warp tests share.  Everything takes ONE utterance.

    n_out = min(max(n_out_in, 1), N_out)
    u = (s_j >> 8) / hop_out, fr = s_j - u hop_out Q, lin = tmap[u] + ((tmap[u + 1] - tmap[u]) fr) / (hop_out Q)    (truncating)
    ta_j = min(max(lin, ta_{j-1}, 0), Q n - 1)
    r_j = ratio[frame(ta_j)] (axis 0) or ratio[min(RT - 1, n_out / hop_out, ((s_j >> 8) + hop_out / 2) / hop_out)] (axis 1), clamped
    s_{j+1} = s_j + max(8 Q, rint(float(per[frame(ta_j)]) / r_j)) on a voiced frame(ta_j), + unvoiced_period Q otherwise

    time map of a path: mid_j = 128 hop (lo_j + hi_j), tmap[u] = (sum over d = -w ..= w of mid[clamp(u + d, 0, J - 1)]) / (2 w + 1)"""
import numpy as np

import prosody_ref as R
from flowtron_amd import prosody as PR

Q = 256
MAX_SAMPLES = 1 << 22


def _trunc_div(a, b):
    """a / b toward zero, b > 0 (Python's // floors)"""
    return a // b if a >= 0 else -((-a) // b)


def marks_warp(f0, n, sr, hop, tmap, n_out, ratio=1.0, ratio_axis=0, hop_out=None, unvoiced_period=None, N_out=None, dtype=np.float32):
    """f0 [T] Hz of ONE utterance of n samples, tmap [TM] integers -> dict(analysis, synthesis, source, half int32, n_out).
    ratio: a number, or [T] on the input's frames (axis 0), or [RT] on the output's (axis 1).  N_out: the row's width (None:
    n_out itself)."""
    dtype = np.dtype(dtype).type
    T = len(f0)
    assert T >= n // hop + 1
    hop_out = hop if hop_out is None else int(hop_out)
    unv = PR.default_unvoiced_period(sr) if unvoiced_period is None else int(unvoiced_period)
    n_out = min(max(int(n_out), 1), max(int(n_out), 1) if N_out is None else int(N_out))
    tmap = [int(v) for v in np.asarray(tmap).tolist()]
    assert len(tmap) >= (n_out - 1) // hop_out + 2
    T = min(T, n // hop + 1)                                                 # no frame above n / hop is read
    f0 = np.asarray(f0, dtype)[:T]
    if ratio_axis == 0:
        per, step = R._periods(f0, ratio if np.ndim(ratio) == 0 else np.asarray(ratio)[:T], sr, unv, dtype)
    else:
        per, _ = R._periods(f0, 1.0, sr, unv, dtype)
        r_out = np.asarray(ratio, dtype).reshape(-1)
        if np.ndim(ratio) == 0:
            r_out = np.full(n_out // hop_out + 1, ratio, dtype)
        r_out = r_out[:n_out // hop_out + 1]                                 # no entry above n_out / hop_out is read
        r_out = np.where(r_out >= dtype(PR.MIN_RATIO), r_out, dtype(PR.MIN_RATIO))
        r_out = np.where(r_out <= dtype(PR.MAX_RATIO), r_out, dtype(PR.MAX_RATIO)).astype(dtype)
        step = None
    voiced = (np.isfinite(f0) & (f0 > 0)).tolist()
    per = per.tolist()
    step = step.tolist() if step is not None else None

    def frame(p):
        return min(T - 1, ((p >> 8) + hop // 2) // hop)

    a = [0]
    while True:
        nxt = a[-1] + per[frame(a[-1])]
        if (nxt >> 8) >= n:
            break
        a.append(nxt)
    K = len(a)
    s, syn, src, half, k, ta = 0, [], [], [], 0, 0
    den = hop_out * Q
    while (s >> 8) < n_out:
        u = (s >> 8) // hop_out
        fr = s - u * den
        lin = tmap[u] + _trunc_div((tmap[u + 1] - tmap[u]) * fr, den)
        ta = min(max(lin, ta, 0), Q * n - 1)
        while k + 1 < K and abs(a[k + 1] - ta) <= abs(a[k] - ta):
            k += 1
        syn.append(s)
        src.append(k)
        half.append((per[frame(a[k])] + 128) >> 8)
        t = frame(ta)
        if not voiced[t]:
            s += unv * Q
        elif ratio_axis == 0:
            s += step[t]
        else:
            r = r_out[min(len(r_out) - 1, ((s >> 8) + hop_out // 2) // hop_out)]
            s += max(8 * Q, int(np.rint(dtype(dtype(per[t]) / r))))
    i32 = lambda v: np.asarray(v, np.int32)
    return dict(analysis=i32(a), synthesis=i32(syn), source=i32(src), half=i32(half), n_out=n_out)


def warp(x, f0, sr, hop, tmap, n_out, ratio=1.0, ratio_axis=0, hop_out=None, unvoiced_period=None, N_out=None, dtype=np.float32):
    """-> (out [n_out], marks): prosody_ref.synth on the marks, unchanged"""
    m = marks_warp(f0, len(x), sr, hop, tmap, n_out, ratio, ratio_axis, hop_out, unvoiced_period, N_out, dtype)
    return R.synth(x, m, dtype), m


def constant_map(pace, hop, entries):
    """tmap[u] = u hop Q pace for a pace whose product is an integer (1, 2, 0.5, ...)"""
    v = np.arange(entries, dtype=np.int64) * hop * Q * pace
    assert np.all(v == np.floor(v))
    return v.astype(np.int64)


def time_map_from_path(path, path_len, hop, TM, w, P=None):
    """path [>= path_len, 2] cells (i, j) of ONE utterance -> tmap [TM] int32.  P: the row's capacity (None: len(path))"""
    path = np.asarray(path, np.int64)
    P = len(path) if P is None else P
    Pb = min(max(int(path_len), 1), P)
    i = np.clip(path[:Pb, 0], 0, (MAX_SAMPLES - 1) // hop)
    j = np.clip(path[:Pb, 1], 0, P - 1)
    J = int(j[-1]) + 1
    lo, hi = np.zeros(J, np.int64), np.zeros(J, np.int64)
    for c in range(Pb):
        if j[c] < J and (c == 0 or j[c - 1] != j[c]):
            lo[j[c]] = i[c]
        if j[c] < J and (c == Pb - 1 or j[c + 1] != j[c]):
            hi[j[c]] = i[c]
    mid = 128 * hop * (lo + hi)
    out = np.zeros(TM, np.int64)
    for u in range(TM):
        out[u] = int(sum(int(mid[min(max(u + d, 0), J - 1)]) for d in range(-w, w + 1))) // (2 * w + 1)
    return out.astype(np.int32)


def time_map_from_durations(src, tgt, hop, U):
    """token durations of ONE utterance -> (tmap [U] int32, the target's frames): tmap[u] = Qh S_l + (Qh d_l (u - E_l)) // e_l for
    E_l <= u < E_{l+1}, Qh S_total at and behind the target's total"""
    src, tgt = [max(int(v), 0) for v in src], [max(int(v), 0) for v in tgt]
    qh = Q * hop
    out = []
    for u in range(U):
        S = E = 0
        val = None
        for d, e in zip(src, tgt):
            if E <= u < E + e:
                val = qh * S + (qh * d * (u - E)) // e
                break
            S, E = S + d, E + e
        out.append(min(max(qh * sum(src) if val is None else val, 0), 2 ** 31 - 1))
    return np.asarray(out, np.int32), sum(tgt)


def transfer_ratio(f0_src, f0_ref, tmap, hop, register="reference"):
    """float64 statement of prosody.transfer_ratio for one utterance -> [T_ref] float32"""
    fs, fr = np.asarray(f0_src, np.float64), np.asarray(f0_ref, np.float64)
    vs, vr = np.isfinite(fs) & (fs > 0), np.isfinite(fr) & (fr > 0)
    tm = np.asarray(tmap, np.int64)[:len(fr)]
    t = np.clip(((tm >> 8) + hop // 2) // hop, 0, len(fs) - 1)
    both = vr & vs[t]
    c = 1.0
    if register == "source" and vs.any() and vr.any():
        c = 2.0 ** (np.log2(fs[vs]).mean() - np.log2(fr[vr]).mean())
    with np.errstate(all="ignore"):
        return np.where(both, (np.where(both, fr, 1.0) * c) / np.where(both, fs[t], 1.0), 1.0).astype(np.float32)


# ---- the transfer signal: one sentence said twice, the second time with another rhythm and another melody -------------------------
SR, HOP = 8000, 80
N_SRC, N_REF = 8000, 9600


def _voice(f, tau, seed):
    """harmonics below 3600 Hz of the contour f (Hz per sample) with prosody_ref's envelope, amplitude 0.6 + 0.4 sin(2 pi 5 tau),
    silent for content time tau in [0.4, 0.6), noise 0.005"""
    rng = np.random.RandomState(seed)
    n = len(f)
    phase = 2 * np.pi * np.cumsum(f) / SR
    x = np.zeros(n)
    for h in range(1, 26):
        hf = h * f
        ph = -np.arctan((hf - 600.0) / 150.0) - np.arctan((hf - 1700.0) / 250.0)
        x += np.where(hf < 3600.0, R.env(hf) * np.cos(h * phase + ph), 0.0)
    x *= 0.3 / np.abs(x).max()
    x *= 0.6 + 0.4 * np.sin(2 * np.pi * 5.0 * tau)
    x[(tau >= 0.4) & (tau < 0.6)] = 0.0
    return (x + 0.005 * rng.randn(n)).astype(np.float32)


def content_time(v):
    """the content time the reference is at, at v = n / N_REF of its length"""
    v = np.asarray(v, np.float64)
    return v + 0.08 * np.sin(2 * np.pi * v)


def reference_f0(v):
    v = np.asarray(v, np.float64)
    return 170.0 * 2.0 ** (-0.35 * v + 0.02 * np.sin(2 * np.pi * 4.0 * v))


_SIGNAL = {}


def transfer_signal():
    """-> dict(src [8000], ref [9600] float32, truth [121] Hz: the reference's contour at its frames' centres, voiced [121] bool,
    true_map [121]: the source sample the reference's frame plays), made once"""
    if not _SIGNAL:
        tau_s = np.arange(N_SRC) / N_SRC
        src = _voice(R.glide_f0(np.arange(N_SRC) / SR), tau_s, 1)
        v = np.arange(N_REF) / N_REF
        ref = _voice(reference_f0(v), content_time(v), 2)
        at = np.arange(N_REF // HOP + 1) * HOP / N_REF
        tau = content_time(at)
        _SIGNAL.update(src=src, ref=ref, truth=reference_f0(at), voiced=~((tau >= 0.4) & (tau < 0.6)) & (at < 1.0), true_map=tau * N_SRC)
    return _SIGNAL


def log_power(x, frame=160, hop=HOP):
    """log of the mean square of `frame`-sample frames at `hop`, frame t centred on sample t hop as the frames of F0 are (zeros
    outside the signal), floor 1e-10 -> [len(x) // hop + 1, 1] float32: the one feature the transfer test warps along"""
    x = np.asarray(x, np.float64)
    T = len(x) // hop + 1
    pad = np.concatenate([np.zeros(frame // 2), x, np.zeros(frame + hop)])
    p = np.array([np.mean(pad[t * hop:t * hop + frame] ** 2) for t in range(T)])
    return np.log(np.maximum(p, 1e-10)).astype(np.float32)[:, None]
