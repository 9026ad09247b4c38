"""The single-pass phase start (ft_spsi_phase, csrc/vocode.hip) beside the Griffin-Lim loop it shortens: device-event time of whole
warm calls on four utterances of 862 / 640 / 410 / 200 frames and on 64 x 862 frames at 1024 / 256, 80 bands, NNLS inversion:
ft_spsi_phase alone, the zero-iteration vocode from SPSI, 5 iterations from SPSI, 30 iterations from the random start (angles
already on the device) and one Griffin-Lim iteration of the same batch; median of repeated runs, one process.  Then the round
trip's mean |log-mel error| of the four utterances for 0, 5 and 30 plain iterations from both starts.
usage: timeout -k 10 600 python scripts/prof_spsi.py [--reps R] [--out profiles/spsi_prof.txt]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import audio_processing
from flowtron_amd import _lib as L
from oracle import synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
a = ap.parse_args()
tst = audio_processing.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).cuda()
T = 862
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.array(ms)


def batch(lens):
    """Log-mels [B, 80, T] of synthetic utterances of these lengths (8 different signals, repeated), zeros behind each."""
    mel = torch.zeros(len(lens), 80, T, device="cuda")
    own = {}
    for b, n in enumerate(lens):
        key = (n, b % 8)
        if key not in own:
            own[key] = tst.mel_spectrogram(synth.make_audio(256 * (n - 1), seed=b % 8)[None].cuda())[0]
        mel[b, :, :n] = own[key]
    return mel


for lens in ([862, 640, 410, 200], [T] * 64):
    B = len(lens)
    mel = batch(lens)
    ang = (torch.rand(B, 513, T, device="cuda") * 2 - 1) * np.pi
    what = "4 utterances %s" % lens if B == 4 else "%d x %d frames" % (B, T)
    mag = tst.mel_to_magnitude(mel, method="nnls", lengths=lens)
    nf = torch.tensor(lens, dtype=torch.int32, device="cuda")
    out = torch.empty_like(mag)

    def spsi():
        L.check(L.lib().ft_spsi_phase(L.ptr(mag), L.ptr(out), L.ptr(nf), B, 1024, 256, T, L.stream()), "ft_spsi_phase")
    ms = timed(spsi) * 1e3
    say("ft_spsi_phase %s: median %.1f us (min %.1f, max %.1f, %d runs) = %.3f us per frame of the longest utterance"
        % (what, np.median(ms), ms.min(), ms.max(), a.reps, np.median(ms) / max(lens)))
    kw = dict(inversion="nnls", lengths=lens)
    gl = {}
    for name, fn in (("0 iterations from SPSI", lambda: tst.mel_to_audio(mel, 0, phase_init="spsi", **kw)),
                     ("5 iterations from SPSI", lambda: tst.mel_to_audio(mel, 5, phase_init="spsi", **kw)),
                     ("0 iterations from given angles", lambda: tst.mel_to_audio(mel, 0, angles=ang, **kw)),
                     ("30 iterations from given (random) angles", lambda: tst.mel_to_audio(mel, 30, angles=ang, **kw))):
        ms = timed(fn)
        gl[name] = float(np.median(ms))
        say("mel_to_audio(inversion='nnls', lengths=) %s, %s: median %.3f ms (min %.3f, max %.3f, %d runs)"
            % (what, name, np.median(ms), ms.min(), ms.max(), a.reps))
    one = (gl["30 iterations from given (random) angles"] - gl["0 iterations from given angles"]) / 30
    say("one plain Griffin-Lim iteration of %s: %.1f us (the difference of the two calls above / 30)" % (what, one * 1e3))
    if B == 4:
        for n_iters in (0, 5, 30):
            err = {}
            for start in ("random", "spsi"):
                np.random.seed(0)
                y = tst.mel_to_audio(mel, n_iters, phase_init=start, **kw)
                tot, cells = 0.0, 0
                for b, n in enumerate(lens):
                    back = tst.mel_spectrogram(y[b:b + 1, :256 * (n - 1)])
                    tot += float((back - mel[b:b + 1, :, :n]).abs().double().sum())
                    cells += back.numel()
                err[start] = tot / cells
            say("round trip of %s, NNLS, %d plain iterations: mean |log-mel error| %.4f from the random start, %.4f from SPSI"
                % (what, n_iters, err["random"], err["spsi"]))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
