"""Mel -> waveform with the NNLS mel inversion (ft_mel_nnls) and the fast Griffin-Lim step (ft_gl_momentum), csrc/vocode.hip:
device-event time of whole warm mel_to_audio(..., lengths=) calls (mel_to_audio_ragged's pass; starting angles already on the
device) on four utterances of 862 / 640 / 410 / 200 frames and on 64 x 862 frames at 1024 / 256, 80 bands, for
pinv + plain, NNLS + plain, pinv + momentum and NNLS + momentum, and of the two kernels alone; median of repeated runs.
usage: python scripts/prof_vocode.py [--reps R] [--out profiles/vocode_prof.txt]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import audio_processing
from flowtron_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--n-iters", type=int, default=30)
ap.add_argument("--nnls-iters", type=int, default=100)
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


MODES = [("pinv + plain", dict()), ("NNLS + plain", dict(inversion="nnls", inversion_iters=a.nnls_iters)),
         ("pinv + momentum", dict(momentum=0.99)),
         ("NNLS + momentum", dict(momentum=0.99, inversion="nnls", inversion_iters=a.nnls_iters))]
for lens in ([862, 640, 410, 200], [T] * 64):
    B = len(lens)
    mel = torch.rand(B, 80, T, device="cuda") * 9.5 - 9.0
    ang = (torch.rand(B, 513, T, device="cuda") * 2 - 1) * np.pi
    what = "4 utterances %s" % lens if B == 4 else "%d x %d frames" % (B, T)
    for name, kw in MODES:
        ms = timed(lambda: tst.mel_to_audio(mel, a.n_iters, lengths=lens, angles=ang, **kw))
        say("mel_to_audio(lengths=) %s, n_iters=%d, %s: median %.3f ms (min %.3f, max %.3f, %d runs)"
            % (what, a.n_iters, name, np.median(ms), ms.min(), ms.max(), a.reps))
    # the two kernels alone
    s = torch.exp(mel).contiguous()
    m0 = tst.mel_to_magnitude(mel)
    out = torch.empty_like(m0)
    band, weight = tst._bin_table(mel.device)
    nf = torch.tensor(lens, dtype=torch.int32, device="cuda")

    def nnls():
        L.check(L.lib().ft_mel_nnls(L.ptr(s), L.ptr(m0), L.ptr(out), L.ptr(nf), L.ptr(tst.fb_bin0), L.ptr(tst.fb_ptr), L.ptr(tst.fb_w),
                                    L.ptr(band), L.ptr(weight), B, 80, 1024, T, tst.fb_w.numel(), a.nnls_iters, L.stream()), "ft_mel_nnls")
    ms = timed(nnls)
    say("ft_mel_nnls %s, %d iterations: median %.3f ms (min %.3f, max %.3f, %d runs)"
        % (what, a.nnls_iters, np.median(ms), ms.min(), ms.max(), a.reps))
    prev = torch.zeros(2, B, 513, T, device="cuda")
    ph = ang.clone()

    def step():
        L.check(L.lib().ft_gl_momentum(L.ptr(m0), L.ptr(ph), L.ptr(prev[0]), L.ptr(prev[1]), L.ptr(nf), B, 513, T, 0.99, 0, L.stream()),
                "ft_gl_momentum")
    ms = timed(step) * 1e3
    cells = 513 * sum(lens)
    say("ft_gl_momentum %s: median %.1f us (min %.1f, max %.1f, %d runs), %.1f MB at 28 bytes a cell, %.0f GB/s algorithmic"
        % (what, np.median(ms), ms.min(), ms.max(), a.reps, 28 * cells / 1e6, 28 * cells / (np.median(ms) * 1e-6) / 1e9))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
