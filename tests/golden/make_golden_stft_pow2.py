"""Golden vectors for the power-of-two analysis sizes of the audio front end: the REAL reference's TacotronSTFT.mel_spectrogram,
STFT.transform, STFT.inverse, griffin_lim and window_sumsquare (audio_processing.py:7-75, 96-270) on CPU, with make_golden.py's
librosa stub, at three data_config settings of other sample rates (sampling_rate, filter_length, hop_length, win_length):

  sr16k    (16000, 512, 128, 512)
  sr24k    (24000, 2048, 300, 1200)
  sr44k    (44100, 2048, 512, 2048)

Run once in the build container:   python tests/golden/make_golden_stft_pow2.py   ->   tests/golden/stft_pow2.pt

Inputs are not stored: audio comes from oracle/synth.py, random spectra from np.random.RandomState seeds, and the Griffin-Lim
magnitudes are |STFT| of synth audio in float64 rounded to float32 (`magnitudes32`; the fixture keeps a fingerprint).  Every
case records the reference's own relative-L2 deviation from a float64 restatement of the same formula (`dev64`), the yardstick
tests/test_gpu_stft_pow2.py holds the device code to.  Long outputs are kept as every STRIDE-th sample or column.

Per setting:
  mel        TacotronSTFT(n_fft, hop, win, 80, sr, 0, 8000).mel_spectrogram of one synth clip (60 hops long)
  transform  STFT.transform magnitude, every MAG_STRIDE-th frame
  inverse    STFT.inverse on a seeded random spectrum (magnitude in [0, 2), phase in [-pi, pi)), B = 1, T = 12
  gl         griffin_lim under np.random.seed(0) at 0 / 1 / 8 iterations of a 30-frame synth clip's magnitudes
  wss        window_sumsquare for 12 frames
"""
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
SETTINGS = {"sr16k": (16000, 512, 128, 512), "sr24k": (24000, 2048, 300, 1200), "sr44k": (44100, 2048, 512, 2048)}
MAG_STRIDE, Y_STRIDE, GL_ITERS = 10, 8, (0, 1, 8)


def hann64(win_length, n_fft):
    w = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    w[lp:lp + win_length] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)
    return w


def transform64(y, n_fft, hop, win_length):
    """complex STFT [B, n_fft/2+1, N // hop + 1] of the reflect-padded, hann-windowed signal, float64."""
    B, N = y.shape
    w = hann64(win_length, n_fft)
    yp = np.pad(np.asarray(y, np.float64), ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    idx = np.arange(N // hop + 1)[:, None] * hop + np.arange(n_fft)[None, :]
    return np.fft.rfft(yp[:, idx] * w, axis=2).transpose(0, 2, 1)


def istft64(M, P, n_fft, hop, win_length):
    B, _, T = M.shape
    w = hann64(win_length, n_fft)
    fr = np.fft.irfft(np.asarray(M, np.float64) * np.exp(1j * np.asarray(P, np.float64)), n=n_fft, axis=1) * w[None, :, None]
    n = n_fft + hop * (T - 1)
    out, wss = np.zeros((B, n)), np.zeros(n)
    for t in range(T):
        out[:, t * hop:t * hop + n_fft] += fr[:, :, t]
        wss[t * hop:t * hop + n_fft] += w * w
    nz = wss > TINY32
    out[:, nz] /= wss[nz]
    return out[:, n_fft // 2:n - n_fft // 2]


def magnitudes32(y, n_fft, hop, win_length):
    return np.abs(transform64(y, n_fft, hop, win_length)).astype(np.float32)


def random_spectrum(seed, B, T, n_fft):
    rs = np.random.RandomState(seed)
    M = rs.uniform(0.0, 2.0, (B, n_fft // 2 + 1, T)).astype(np.float32)
    P = rs.uniform(-np.pi, np.pi, (B, n_fft // 2 + 1, T)).astype(np.float32)
    return M, P


def start_angles(shape):
    np.random.seed(0)
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32)


def griffin_lim64(M, angles, n_iters, n_fft, hop, win_length):
    y = istft64(M, angles, n_fft, hop, win_length)
    for _ in range(n_iters):
        y = istft64(M, np.angle(transform64(y, n_fft, hop, win_length)), n_fft, hop, win_length)
    return y


def fingerprint(M):
    return {"sum64": float(np.asarray(M, np.float64).sum()), "sample": torch.from_numpy(np.ascontiguousarray(M.reshape(-1)[::997]))}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    assert refshim.available(), "needs the reference checkout"
    torch.set_num_threads(8)
    stub_librosa()
    sys.path.insert(0, refshim.REF_DIR)
    import audio_processing as AP  # the reference module

    res = {"settings": SETTINGS, "mag_stride": MAG_STRIDE, "y_stride": Y_STRIDE}
    for ci, (name, (sr, n_fft, hop, win)) in enumerate(SETTINGS.items()):
        case = {}
        # mel_spectrogram
        seed, n = 10 + ci, hop * 60
        y = synth.make_audio(n, seed=seed)[None]
        tst = AP.TacotronSTFT(n_fft, hop, win, 80, sr, 0.0, 8000.0)
        with torch.no_grad():
            mel = tst.mel_spectrogram(y)
        basis = tst.mel_basis.double().numpy()
        mel64 = np.log(np.maximum(basis @ np.abs(transform64(y.numpy(), n_fft, hop, win))[0], 1e-5))
        case["mel"] = {"audio_seed": seed, "n_samples": n, "mel": mel[0].clone(), "dev64": rel_l2(mel[0].numpy(), mel64)}
        # STFT.transform
        st = AP.STFT(n_fft, hop, win)
        with torch.no_grad():
            mag, _ = st.transform(y)
        mag64 = np.abs(transform64(y.numpy(), n_fft, hop, win))
        case["transform"] = {"audio_seed": seed, "n_samples": n, "mag": mag[0, :, ::MAG_STRIDE].clone(),
                             "dev64": rel_l2(mag.numpy(), mag64)}
        # STFT.inverse
        sseed = 20 + ci
        M, P = random_spectrum(sseed, 1, 12, n_fft)
        with torch.no_grad():
            yi = st.inverse(torch.from_numpy(M), torch.from_numpy(P))[:, 0]
        case["inverse"] = {"seed": sseed, "B": 1, "T": 12, "y": yi[:, ::Y_STRIDE].clone(),
                           "dev64": rel_l2(yi.numpy(), istft64(M, P, n_fft, hop, win))}
        # griffin_lim
        gseed = 30 + ci
        Mg = magnitudes32(synth.make_audio(hop * 29, seed=gseed)[None].numpy(), n_fft, hop, win)
        g = {"audio_seed": gseed, "n_samples": hop * 29, "mag": fingerprint(Mg), "n_iters": list(GL_ITERS), "y": {}, "dev64": {}}
        for it in GL_ITERS:
            np.random.seed(0)
            with torch.no_grad():
                out = AP.griffin_lim(torch.from_numpy(Mg), st, it)
            g["y"][it] = out[:, ::Y_STRIDE].clone()
            g["dev64"][it] = rel_l2(out.numpy(), griffin_lim64(Mg, start_angles(Mg.shape), it, n_fft, hop, win))
        case["gl"] = g
        case["wss"] = {"args": dict(n_frames=12, hop_length=hop, win_length=win, n_fft=n_fft),
                       "out": torch.from_numpy(AP.window_sumsquare("hann", 12, hop_length=hop, win_length=win, n_fft=n_fft,
                                                                   dtype=np.float32))}
        res[name] = case
        print(name, "dev64: mel %.2e transform %.2e inverse %.2e" % (case["mel"]["dev64"], case["transform"]["dev64"],
                                                                    case["inverse"]["dev64"]),
              "gl", {k: "%.2e" % v for k, v in g["dev64"].items()})

    path = os.path.join(HERE, "stft_pow2.pt")
    torch.save(res, path)
    print("stft_pow2.pt", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
