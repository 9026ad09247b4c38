"""Golden vectors for the synthesis side of the audio front end: the REAL reference's STFT.inverse, griffin_lim and
window_sumsquare (audio_processing.py:7-75, 237-270) on CPU, with make_golden.py's librosa stub.

Run once in the build container:   python tests/golden/make_golden_gl.py   ->   tests/golden/griffin_lim.pt

Inputs are not stored: the random spectra come from np.random.RandomState seeds, and the Griffin-Lim magnitudes are
|STFT| of oracle/synth.py audio computed in float64 and rounded to float32 (`magnitudes32`, restated in the test; the fixture
keeps a fingerprint so the test can prove it rebuilt the same input).  Every case records the reference's own deviation
from a float64 restatement of the same formula (relative L2, `dev64`): that deviation is the yardstick
tests/test_gpu_griffin_lim.py holds the device code to.  The restatement here is the generator's own copy; the test carries
another.  Long outputs are kept as every STRIDE-th sample.

  inverse_h256 / inverse_h200   STFT.inverse on random magnitude and phase (phase of bins 0 and 512 not zero)
  gl_41                         griffin_lim under np.random.seed(0) at 0 / 1 / 8 / 32 iterations, 2 x 41-frame synth clips
  gl_862                        griffin_lim under np.random.seed(0), 30 iterations, one 862-frame (10 s) clip
  wss                           window_sumsquare for (n_fft, hop, win_length) = (1024, 256, 1024) and (1024, 200, 800)
  signatures                    the reference's signatures of these functions
"""
import inspect
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import stub_librosa  # noqa: E402
from oracle import refshim, synth  # noqa: E402

TINY32 = float(np.finfo(np.float32).tiny)
STRIDE = {"gl_41": 8, "gl_862": 64}


def random_spectrum(seed, B, T):
    """STFT.inverse inputs: magnitude in [0, 2), phase in [-pi, pi) (bins 0 and 512 included), float32."""
    rs = np.random.RandomState(seed)
    M = rs.uniform(0.0, 2.0, (B, 513, T)).astype(np.float32)
    P = rs.uniform(-np.pi, np.pi, (B, 513, T)).astype(np.float32)
    return M, P


def hann64(win_length, n_fft):
    w = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    w[lp:lp + win_length] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)
    return w


def istft64(M, P, hop, win_length):
    """y[n] = sum_t w irfft(M e^{iP})[n + 512 - t hop] / wss[n + 512] (where wss > tiny), float64."""
    B, _, T = M.shape
    w = hann64(win_length, 1024)
    fr = np.fft.irfft(M.astype(np.float64) * np.exp(1j * P.astype(np.float64)), n=1024, axis=1) * w[None, :, None]
    n = 1024 + hop * (T - 1)
    out, wss = np.zeros((B, n)), np.zeros(n)
    for t in range(T):
        out[:, t * hop:t * hop + 1024] += fr[:, :, t]
        wss[t * hop:t * hop + 1024] += w * w
    nz = wss > TINY32
    out[:, nz] /= wss[nz]
    return out[:, 512:n - 512]


def transform64(y, hop, win_length):
    B, N = y.shape
    w = hann64(win_length, 1024)
    yp = np.pad(y.astype(np.float64), ((0, 0), (512, 512)), mode="reflect")
    T = N // hop + 1
    idx = np.arange(T)[:, None] * hop + np.arange(1024)[None, :]
    X = np.fft.rfft(yp[:, idx] * w, axis=2).transpose(0, 2, 1)            # [B, 513, T]
    return np.abs(X), np.angle(X)


def magnitudes32(y, hop=256, win_length=1024):
    """The Griffin-Lim input: |STFT(y)| in float64, rounded once to float32."""
    return transform64(np.asarray(y, np.float64), hop, win_length)[0].astype(np.float32)


def fingerprint(M):
    return {"sum64": float(np.asarray(M, np.float64).sum()), "sample": torch.from_numpy(np.ascontiguousarray(M.reshape(-1)[::997]))}


def griffin_lim64(M, angles, n_iters, hop, win_length):
    y = istft64(M, angles, hop, win_length)
    for _ in range(n_iters):
        _, ph = transform64(y, hop, win_length)
        y = istft64(M, ph, hop, win_length)
    return y


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def spectral_convergence(y, M, hop, win_length):
    mag, _ = transform64(np.asarray(y, np.float64), hop, win_length)
    return float(np.linalg.norm(mag - M) / np.linalg.norm(M))


def start_angles(shape):
    """griffin_lim's draw (audio_processing.py:67-68) after np.random.seed(0)."""
    np.random.seed(0)
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32)


def main():
    assert refshim.available(), "needs the reference checkout"
    torch.set_num_threads(8)
    stub_librosa()
    sys.path.insert(0, refshim.REF_DIR)
    import audio_processing as AP  # the reference module

    res = {"signatures": {"griffin_lim": str(inspect.signature(AP.griffin_lim)),
                          "window_sumsquare": str(inspect.signature(AP.window_sumsquare)),
                          "STFT.inverse": str(inspect.signature(AP.STFT.inverse)),
                          "STFT.forward": str(inspect.signature(AP.STFT.forward))}}

    for name, seed, hop, win, B, T in (("inverse_h256", 7, 256, 1024, 2, 20), ("inverse_h200", 8, 200, 800, 1, 17)):
        M, P = random_spectrum(seed, B, T)
        st = AP.STFT(1024, hop, win)
        with torch.no_grad():
            y = st.inverse(torch.from_numpy(M), torch.from_numpy(P))
        y64 = istft64(M, P, hop, win)
        res[name] = {"seed": seed, "B": B, "T": T, "hop": hop, "win_length": win, "y": y[:, 0].clone(),
                     "dev64": rel_l2(y[:, 0].numpy(), y64)}

    stft = AP.STFT(1024, 256, 1024)
    Mn = magnitudes32(torch.stack([synth.make_audio(256 * 40, seed=s) for s in (0, 1)]).numpy())
    M = torch.from_numpy(Mn)
    st41 = STRIDE["gl_41"]
    case = {"audio_seeds": [0, 1], "n_samples": 256 * 40, "mag": fingerprint(Mn), "n_iters": [0, 1, 8, 32], "stride": st41,
            "y": {}, "dev64": {}, "sc_ref": {}, "sc64": {}}
    for n in case["n_iters"]:
        np.random.seed(0)
        with torch.no_grad():
            out = AP.griffin_lim(M, stft, n)
        y64 = griffin_lim64(Mn, start_angles(Mn.shape), n, 256, 1024)
        case["y"][n] = out[:, ::st41].clone()
        case["dev64"][n] = rel_l2(out.numpy(), y64)
        case["sc_ref"][n] = spectral_convergence(out.numpy(), Mn, 256, 1024)
        case["sc64"][n] = spectral_convergence(y64, Mn, 256, 1024)
    res["gl_41"] = case

    Mn = magnitudes32(synth.make_audio(220500, seed=2)[None].numpy())
    M = torch.from_numpy(Mn)
    np.random.seed(0)
    with torch.no_grad():
        out = AP.griffin_lim(M, stft, 30)
    y64 = griffin_lim64(Mn, start_angles(Mn.shape), 30, 256, 1024)
    res["gl_862"] = {"audio_seed": 2, "n_samples": 220500, "mag": fingerprint(Mn), "n_iters": 30, "stride": STRIDE["gl_862"],
                     "y": out[:, ::STRIDE["gl_862"]].clone(), "dev64": rel_l2(out.numpy(), y64),
                     "sc_ref": spectral_convergence(out.numpy(), Mn, 256, 1024), "sc64": spectral_convergence(y64, Mn, 256, 1024)}

    res["wss"] = [{"args": dict(n_frames=nf, hop_length=hop, win_length=win, n_fft=1024),
                   "out": torch.from_numpy(AP.window_sumsquare("hann", nf, hop_length=hop, win_length=win, n_fft=1024,
                                                               dtype=np.float32))}
                  for nf, hop, win in ((41, 256, 1024), (17, 200, 800))]

    path = os.path.join(HERE, "griffin_lim.pt")
    torch.save(res, path)
    print("griffin_lim.pt", os.path.getsize(path) // 1024, "KiB")
    for k in ("inverse_h256", "inverse_h200", "gl_862"):
        print(k, "dev64 %.2e" % res[k]["dev64"])
    print("gl_41 dev64", {n: "%.2e" % v for n, v in res["gl_41"]["dev64"].items()},
          "sc_ref", {n: "%.3f" % v for n, v in res["gl_41"]["sc_ref"].items()})
    print("gl_862 sc_ref %.4f sc64 %.4f" % (res["gl_862"]["sc_ref"], res["gl_862"]["sc64"]))


if __name__ == "__main__":
    main()
