"""Griffin-Lim on the device (audio_processing.griffin_lim: ft_stft_r8 + ft_istft_r8 per iteration) at B = 1 and B = 32 clips
of 862 frames (10 s at 22 050 Hz), n_iters = 30: device-event time of whole calls (they include the reference's host draw
of the starting angles) and of the device loop alone, warm, median and spread of repeated runs.
Then a batch of four utterances of 862 / 640 / 410 / 200 frames: griffin_lim_ragged (ft_stft_r8_ragged_phase + ft_istft_r8_ragged, one
launch per step for the batch) against the loop of four dense runs on the trimmed utterances, device loops from starting angles
already on the device, and whole mel_to_audio_ragged / mel_to_audio calls (they include the host draw of the angles).
A stand-alone workload for rocprofv3 passes too (--reps 1 --warmup 1).  usage: python scripts/prof_griffin_lim.py [--reps R]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import audio_processing

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--n-iters", type=int, default=30)
a = ap.parse_args()
stft = audio_processing.STFT(1024, 256, 1024).cuda()
T, hop = 862, 256
def timed(fn):
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.array(ms)


def loop(mag, signal):
    """griffin_lim's loop body n_iters times (audio_processing.py:71-73): what runs after the host draw of the angles."""
    for _ in range(a.n_iters):
        _, angles = stft.transform(signal)
        signal = stft.inverse(mag, angles).squeeze(1)


for B in (1, 32):
    mag = torch.rand(B, 513, T, device="cuda") * 2
    for _ in range(a.warmup):
        y0 = audio_processing.griffin_lim(mag, stft, a.n_iters)
    torch.cuda.synchronize()
    full = timed(lambda: audio_processing.griffin_lim(mag, stft, a.n_iters))
    it = timed(lambda: loop(mag, y0)) / a.n_iters * 1e3
    n = hop * (T - 1)
    it_bytes = 4 * (2 * B * n + 4 * B * 513 * T)    # transform reads y, writes mag + phase; inverse reads both, writes y
    print("griffin_lim B=%d T=%d n_iters=%d: whole call median %.3f ms (min %.3f, max %.3f, %d runs; includes the host draw of "
          "the starting angles); device loop %.1f us per iteration (min %.1f, max %.1f), %.1f MB per iteration, %.0f GB/s "
          "algorithmic" % (B, T, a.n_iters, np.median(full), full.min(), full.max(), a.reps, np.median(it), it.min(), it.max(),
                           it_bytes / 1e6, it_bytes / (np.median(it) * 1e-6) / 1e9), flush=True)


# ---- a batch of different lengths: one ragged pass against the per-utterance loop ---------------------------------------------
LENS = [862, 640, 410, 200]
tst = audio_processing.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).cuda()
mel = torch.rand(4, 80, T, device="cuda") * 9.5 - 9.0
ang = (torch.rand(4, 513, T, device="cuda") * 2 - 1) * np.pi
mag = tst.mel_to_magnitude(mel)
mels = [mel[b:b + 1, :, :n].contiguous() for b, n in enumerate(LENS)]
mags = [mag[b:b + 1, :, :n].contiguous() for b, n in enumerate(LENS)]
angs = [ang[b:b + 1, :, :n].contiguous() for b, n in enumerate(LENS)]


def dense_from(m, g):
    y = stft.inverse(m, g).squeeze(1)
    for _ in range(a.n_iters):
        _, ph = stft.transform(y)
        y = stft.inverse(m, ph).squeeze(1)
    return y


cases = [("griffin_lim_ragged, angles on the device", lambda: audio_processing.griffin_lim_ragged(mag, LENS, stft, a.n_iters, angles=ang)),
         ("loop of 4 dense runs, angles on the device", lambda: [dense_from(m, g) for m, g in zip(mags, angs)]),
         ("mel_to_audio_ragged (whole call)", lambda: tst.mel_to_audio_ragged(mel, LENS, a.n_iters)),
         ("loop of 4 mel_to_audio (whole calls)", lambda: [tst.mel_to_audio(m, a.n_iters) for m in mels])]
for name, fn in cases:
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ms = timed(fn)
    print("4 utterances %s, n_iters=%d: %s: median %.3f ms (min %.3f, max %.3f, %d runs)"
          % (LENS, a.n_iters, name, np.median(ms), ms.min(), ms.max(), a.reps), flush=True)
