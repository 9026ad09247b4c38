"""The inputs of the inverse STFT's float64 tests, shared by test_istft_ref64_cpu.py (which checks, without a GPU, that the bound
and the wrong inverses of tests/stft_ref64.py mean something on exactly these inputs, and that every case has the geometry
its line claims) and test_gpu_istft_f64.py (which holds istft_r8_k and istft_pow2_k<LH> to them).  Nothing here touches a
device.

A spectrum is M uniform in [0, 2) and phases uniform in [-pi, pi] ([-60, 60] in one case per family), float32, with frame
T // 2 forty times louder than its neighbours; B is 3 so that the batch stride is used."""
import numpy as np

from flowtron_amd.audio import hann_window
from stft_ref64 import TINY32, clamp_frames, default_span, wss64

B = 3
FC_R8, FC_POW2 = 8, 4                                   # frames staged per round (istft_r8_k: FC; istft_pow2_k: one per wave)

# (n_fft, hop, win_length, T, phase range)
R8_CASES = [
    (1024, 256, 1024, 2, np.pi),
    (1024, 256, 1024, 3, np.pi),
    (1024, 256, 1024, 17, np.pi),                        # the output ends on the seam: one full span
    (1024, 256, 1024, 18, np.pi),                        # one hop past it: a span of one hop with three halo frames
    (1024, 255, 1024, 3, 60.0),
    (1024, 13, 1024, 331, np.pi),                        # odd hop, 21 spans, 79 halo frames
    (1024, 7, 800, 2, np.pi),
    (1024, 1, 1024, 2, np.pi),                           # one output sample
    (1024, 1, 1024, 40, np.pi),
    (1024, 1, 1024, 1100, np.pi),                        # t_lo > 0 with the longest halo
    (1024, 256, 256, 5, np.pi),                          # win_length = hop: zero-envelope samples
    (1024, 200, 200, 6, np.pi),
    (1024, 128, 128, 9, np.pi),
]
POW2_CASES = [
    (256, 64, 256, 65, np.pi),                           # one full span
    (256, 64, 256, 66, np.pi),                           # one hop past the seam
    (256, 1, 201, 4300, np.pi),                          # hop 1 across a seam
    (512, 512, 512, 9, np.pi),                           # zero-envelope samples
    (512, 160, 401, 40, 60.0),
    (1024, 257, 1024, 20, np.pi),
    (1024, 512, 512, 12, np.pi),
    (2048, 300, 1200, 15, np.pi),                        # ends 104 samples into the second span
    (4096, 1024, 4096, 5, np.pi),
    (4096, 4096, 4096, 3, np.pi),                        # two spans, zero-envelope samples
    (4096, 333, 3001, 14, np.pi),
    (4096, 1024, 4096, 2, np.pi),
]
CASES = R8_CASES + POW2_CASES


def case_id(c):
    return "n%d_h%d_w%d_T%d" % c[:4]


R8_IDS, POW2_IDS = [case_id(c) for c in R8_CASES], [case_id(c) for c in POW2_CASES]
IDS = R8_IDS + POW2_IDS
BY_ID = dict(zip(IDS, CASES))

# The ragged batches: straight to ft_istft_r8_ragged / ft_istft_pow2_ragged with these counts on the device -- T, the two
# shortest, 0 and T + 5 for the kernels' own clamp (inverse_ragged refuses them on the host), and 17 (at 1024 / 256 the
# utterance ends on the seam, so the second span lies wholly behind it; at 512 / 128 it ends inside the first span).
RAGGED_CASES = [(1024, 256, 1024, 18, np.pi), (512, 128, 512, 48, np.pi)]
RAGGED_IDS = ["ragged_" + case_id(c) for c in RAGGED_CASES]


def ragged_counts(T):
    return [T, 2, 1, 0, T + 5, 17]


def is_r8(n_fft, hop):
    """STFT.fast_path(): the setting istft_r8_k takes."""
    return n_fft == 1024 and hop <= 256


def window32(n_fft, win_length):
    """The float32 window the module hands the kernels."""
    return hann_window(win_length, n_fft)


def spectrum(case, batch=B):
    n_fft, hop, win, T, rng = case
    rs = np.random.RandomState(n_fft + 7 * hop + 13 * win + 31 * T)
    M = rs.uniform(0.0, 2.0, (batch, n_fft // 2 + 1, T)).astype(np.float32)
    P = rs.uniform(-rng, rng, (batch, n_fft // 2 + 1, T)).astype(np.float32)
    M[:, :, T // 2] *= 40.0
    return M, P


def ragged_spectrum(case):
    """(M, P, n_frames): six utterances; NaN in mag and phase behind every clamped length, so a frame read from there shows."""
    T = case[3]
    counts = ragged_counts(T)
    M, P = spectrum(case, batch=len(counts))
    for b, n in enumerate(counts):
        M[b, :, clamp_frames(n, T):] = np.nan
        P[b, :, clamp_frames(n, T):] = np.nan
    return M, P, counts


def geometry(n_fft, hop, T, n_batch_frames=None):
    """What the kernels' index arithmetic makes of an utterance of T frames in a batch of n_batch_frames (default T), restated
    from csrc/stft_r8.hip and csrc/stft_pow2.hip: one dict per workgroup span with n0, the untrimmed range [u0, u1), the
    frames t_lo .. t_hi, `behind` (the early return), `zero_fill` (stored samples with u >= u1), `rounds` / `partial`
    (staging rounds, and whether the last is short) and `halo` (the frames of a later span that start before its first
    sample: its neighbour's, computed again)."""
    H = n_fft // 2
    span, fc = default_span(n_fft, hop), FC_R8 if is_r8(n_fft, hop) else FC_POW2
    n_out = hop * ((T if n_batch_frames is None else n_batch_frames) - 1)
    own = hop * (T - 1)
    out = []
    for n0 in range(0, n_out, span):
        nz1 = min(n0 + span, n_out)
        if n0 >= own:
            out.append(dict(n0=n0, behind=True, zero_fill=nz1 - n0))
            continue
        u0, u1 = n0 + H, min(n0 + span, own) + H
        t_lo = 0 if u0 - (n_fft - 1) <= 0 else -(-(u0 - (n_fft - 1)) // hop)
        t_hi = min(T - 1, (u1 - 1) // hop)
        nfr = t_hi - t_lo + 1
        out.append(dict(n0=n0, behind=False, u0=u0, u1=u1, t_lo=t_lo, t_hi=t_hi, zero_fill=nz1 - (u1 - H),
                        rounds=-(-nfr // fc), partial=nfr % fc != 0,
                        halo=sum(1 for t in range(t_lo, t_hi + 1) if t * hop < u0) if n0 else 0))
    return out


def zero_envelope(n_fft, hop, win, T):
    """The output samples whose envelope is <= tiny(float32), from the float32 window."""
    H = n_fft // 2
    wss = wss64(T, n_fft, hop, win, window32(n_fft, win))
    return wss[H:wss.size - H] <= TINY32


# ---- what every case is on the list for (test_istft_ref64_cpu.py computes each from geometry() and zero_envelope()):
# spans, zero-envelope samples, the largest t_lo, the most halo frames of a span (frames that start before the span's first
# output sample), the most staging rounds, and whether some span's last round is short.
EXPECT = {
    "n1024_h256_w1024_T2": dict(spans=1, zeros=0, t_lo=0, halo=0, rounds=1, partial=True),
    "n1024_h256_w1024_T3": dict(spans=1, zeros=0, t_lo=0, halo=0, rounds=1, partial=True),
    "n1024_h256_w1024_T17": dict(spans=1, zeros=0, t_lo=0, halo=0, rounds=3, partial=True),
    "n1024_h256_w1024_T18": dict(spans=2, zeros=0, t_lo=15, halo=3, rounds=3, partial=True),
    "n1024_h255_w1024_T3": dict(spans=1, zeros=0, t_lo=0, halo=0, rounds=1, partial=True),
    "n1024_h13_w1024_T331": dict(spans=21, zeros=0, t_lo=281, halo=79, rounds=12, partial=True),
    "n1024_h7_w800_T2": dict(spans=1, zeros=0, t_lo=0, halo=0, rounds=1, partial=True),
    "n1024_h1_w1024_T2": dict(spans=1, zeros=0, t_lo=0, halo=0, rounds=1, partial=True),
    "n1024_h1_w1024_T40": dict(spans=3, zeros=0, t_lo=0, halo=40, rounds=5, partial=False),
    "n1024_h1_w1024_T1100": dict(spans=69, zeros=0, t_lo=577, halo=1023, rounds=130, partial=True),
    "n1024_h256_w256_T5": dict(spans=1, zeros=4, t_lo=0, halo=0, rounds=1, partial=True),
    "n1024_h200_w200_T6": dict(spans=1, zeros=5, t_lo=0, halo=0, rounds=1, partial=True),
    "n1024_h128_w128_T9": dict(spans=1, zeros=8, t_lo=0, halo=0, rounds=2, partial=True),
    "n256_h64_w256_T65": dict(spans=1, zeros=0, t_lo=0, halo=0, rounds=17, partial=True),
    "n256_h64_w256_T66": dict(spans=2, zeros=0, t_lo=63, halo=3, rounds=17, partial=True),
    "n256_h1_w201_T4300": dict(spans=2, zeros=0, t_lo=3969, halo=255, rounds=1056, partial=True),
    "n512_h512_w512_T9": dict(spans=1, zeros=8, t_lo=0, halo=0, rounds=3, partial=True),
    "n512_h160_w401_T40": dict(spans=2, zeros=0, t_lo=25, halo=3, rounds=7, partial=True),
    "n1024_h257_w1024_T20": dict(spans=2, zeros=0, t_lo=14, halo=4, rounds=5, partial=True),
    "n1024_h512_w512_T12": dict(spans=2, zeros=11, t_lo=8, halo=1, rounds=3, partial=True),
    "n2048_h300_w1200_T15": dict(spans=2, zeros=0, t_lo=11, halo=4, rounds=4, partial=True),
    "n4096_h1024_w4096_T5": dict(spans=1, zeros=0, t_lo=0, halo=0, rounds=2, partial=True),
    "n4096_h4096_w4096_T3": dict(spans=2, zeros=2, t_lo=1, halo=1, rounds=1, partial=True),
    "n4096_h333_w3001_T14": dict(spans=2, zeros=0, t_lo=7, halo=7, rounds=4, partial=True),
    "n4096_h1024_w4096_T2": dict(spans=1, zeros=0, t_lo=0, halo=0, rounds=1, partial=True),
}

# ---- the wrong inverses (stft_ref64.ISTFT_MUTATIONS) and the cases each must leave the bound on, per family
# (drop_first_halo needs a halo frame whose window taps on the span are not small: at hop 13 and hop 1 the first halo frame
# reaches the span with its last few taps only, ~1e-4 and less, and dropping it stays inside any fp32 bound.  wss_batch_T
# concerns the ragged form alone: RAGGED_IDS.)
MUTATION_CASES = {
    "r8": {
        "drop_first_halo": ["n1024_h256_w1024_T18"],
        "wss_short": ["n1024_h256_w1024_T2", "n1024_h256_w1024_T18", "n1024_h13_w1024_T331", "n1024_h1_w1024_T40",
                      "n1024_h256_w256_T5"],
        "wss_batch_T": [RAGGED_IDS[0]],
        "trim_shift": ["n1024_h256_w1024_T17", "n1024_h7_w800_T2", "n1024_h1_w1024_T2", "n1024_h1_w1024_T1100"],
        "divide_always": ["n1024_h256_w256_T5", "n1024_h200_w200_T6", "n1024_h128_w128_T9"],
        "divide_late": ["n1024_h256_w256_T5", "n1024_h200_w200_T6", "n1024_h128_w128_T9"],
        "symmetric_hann": ["n1024_h256_w1024_T18", "n1024_h13_w1024_T331", "n1024_h256_w256_T5"],
        "window_uncentred": ["n1024_h7_w800_T2", "n1024_h200_w200_T6"],
        "keep_im_dc_nyquist": ["n1024_h256_w1024_T3", "n1024_h255_w1024_T3", "n1024_h1_w1024_T1100"],
    },
    "pow2": {
        "drop_first_halo": ["n256_h64_w256_T66", "n512_h160_w401_T40", "n1024_h257_w1024_T20", "n1024_h512_w512_T12",
                            "n4096_h4096_w4096_T3"],
        "wss_short": ["n256_h64_w256_T65", "n256_h1_w201_T4300", "n2048_h300_w1200_T15", "n4096_h1024_w4096_T2"],
        "wss_batch_T": [RAGGED_IDS[1]],
        "trim_shift": ["n256_h64_w256_T65", "n256_h1_w201_T4300", "n4096_h333_w3001_T14"],
        "divide_always": ["n512_h512_w512_T9", "n1024_h512_w512_T12", "n4096_h4096_w4096_T3"],
        "divide_late": ["n512_h512_w512_T9", "n1024_h512_w512_T12", "n4096_h4096_w4096_T3"],
        "symmetric_hann": ["n256_h64_w256_T66", "n512_h160_w401_T40", "n2048_h300_w1200_T15"],
        "window_uncentred": ["n256_h1_w201_T4300", "n512_h160_w401_T40", "n2048_h300_w1200_T15", "n4096_h333_w3001_T14"],
        "keep_im_dc_nyquist": ["n256_h64_w256_T65", "n1024_h257_w1024_T20", "n4096_h1024_w4096_T5"],
    },
}
ZERO_ENVELOPE_IDS = [i for i in IDS if EXPECT[i]["zeros"]]
