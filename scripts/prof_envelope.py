"""Spectral envelope and mel-cepstra on the device: what a call costs, and how close it comes to the float64 replay.  Whole warm
calls between device events, median of --reps, at 22.05 kHz and a hop of 256 -- 64 utterances of 220,672 samples, the same batch
with LJS-like ragged lengths, and four utterances of 862 / 640 / 410 / 200 frames: envelope.spectral_envelope, envelope.mel_cepstra
with the envelope and without it, metrics.envelope_cepstral_distortion on the batch against its own reverse, and beside them in
the same run pitch.f0_track and metrics.mel_cepstral_distortion.  The NumPy replay (tests/envelope_ref.py) of some utterances on
the host gives the host's time, the conditioning figures (the replay's largest change under input noise of 2^-22 of the peak) and
the device's worst deviation from the replay.  The F0 is pitch.f0_track's.
Writes --out (profiles/envelope_prof.txt).  --resources: appends the compiler's register / LDS / scratch report of the kernels to
--out instead (needs hipcc, no GPU).
usage: python scripts/prof_envelope.py [--reps R] [--warmup W] [--batch B] [--samples N] [--replay-utterances U] [--out FILE] [--resources]"""
import argparse, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--samples", type=int, default=220672)
ap.add_argument("--replay-utterances", type=int, default=4, help="how many utterances the host replays (only their first --replay-frames frames)")
ap.add_argument("--replay-frames", type=int, default=120)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envelope_prof.txt"))
ap.add_argument("--resources", action="store_true")
a = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


if a.resources:
    from flowtron_amd import build
    src = os.path.join(build.CSRC, "envelope.hip")
    r = subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-c", src, "-o", os.devnull,
                                                         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    say("")
    say("== python scripts/prof_envelope.py --resources ==")
    say("compiler resource report, csrc/envelope.hip (%s):" % " ".join(build.FLAGS))
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            k = re.search(r"envelope_kILi(\d+)E", text)
            name = "envelope_k<%s>" % k.group(1) if k else text
            row = []
        elif name and re.match(r"(VGPRs|AGPRs|TotalSGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)", text):
            row.append(text)
            if text.startswith("LDS Size"):
                say("  %-16s %s" % (name, "; ".join(row)))
                name = None
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)

import torch
import envelope_ref as R
import pitch_ref
from flowtron_amd import envelope, metrics, pitch
from flowtron_amd.audio import TacotronSTFT
from oracle import synth

B, N, SR, HOP, ORDER = a.batch, a.samples, 22050, 256, 24
CFG = pitch_ref.DEFAULT


def timed(fn):
    for _ in range(a.warmup):
        fn()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return np.array(ts)


def show(what, t):
    say("  %-84s median %.3f ms (min %.3f, max %.3f, %d calls)" % (what, float(np.median(t)), t.min(), t.max(), len(t)))


def run(name, host, ns, stft):
    Bn = len(ns)
    audio = torch.from_numpy(host[:Bn]).cuda()
    n32 = torch.tensor(ns, dtype=torch.int32).cuda()
    f0 = pitch.f0_track(audio, ns, SR, HOP)[0]
    frames = [n // HOP + 1 for n in ns]
    kw = dict(sampling_rate=SR, hop_length=HOP)
    mc, env = envelope.mel_cepstra(audio, n32, f0, order=ORDER, return_envelope=True, **kw)
    say("%s (%d utterances, %d samples and %d frames in all; %.1f %% of the frames voiced; envelope %.1f MB, mel-cepstra %.1f MB):"
        % (name, Bn, sum(ns), sum(frames), 100.0 * float((f0 > 0).sum()) / float(sum(frames)), env.numel() * 4e-6, mc.numel() * 4e-6))
    show("envelope.spectral_envelope (one launch, a workgroup per frame)", timed(lambda: envelope.spectral_envelope(audio, n32, f0, **kw)))
    show("envelope.mel_cepstra, order 24, with the envelope (the same launch)",
         timed(lambda: envelope.mel_cepstra(audio, n32, f0, order=ORDER, return_envelope=True, **kw)))
    show("envelope.mel_cepstra, order 24, without it (no third transform, no envelope store)",
         timed(lambda: envelope.mel_cepstra(audio, n32, f0, order=ORDER, **kw)))
    if max(frames) <= metrics.MAX_FRAMES:
        rev, rev_n, rev_f0 = torch.flip(audio, [0]), ns[::-1], torch.flip(f0, [0])
        show("metrics.envelope_cepstral_distortion, the batch against its reverse (2 + 1 launches)",
             timed(lambda: metrics.envelope_cepstral_distortion(audio, ns, f0, rev, rev_n, rev_f0, **kw)))
        mel = stft.mel_spectrogram_ragged(audio, n32)
        show("metrics.mel_cepstral_distortion on the log-mels of the same pairs (mels given)",
             timed(lambda: metrics.mel_cepstral_distortion(mel, frames, torch.flip(mel, [0]), frames[::-1])))
    show("pitch.f0_track on the same audio (two launches)", timed(lambda: pitch.f0_track(audio, ns, SR, HOP)))
    U = min(a.replay_utterances, Bn)
    A32 = envelope.freqt_matrix(512, ORDER, envelope.alpha_for(SR)).astype(np.float32)
    f0_h, env_h, mc_h = f0.cpu().numpy(), env[:U].cpu().numpy().astype(np.float64), mc[:U].cpu().numpy().astype(np.float64)
    took, fig_e, fig_m, off_e, off_m, nf = 0.0, 0.0, 0.0, 0.0, 0.0, 0
    for b in range(U):
        n = min(ns[b], (a.replay_frames - 1) * HOP)       # a prefix: every one of its frames is a frame of the whole but the last few,
        T = n // HOP + 1                                   # whose windows the prefix's end cuts; those are left out of the comparison
        keep = T - 3
        x64 = host[b, :n].astype(np.float64)
        t0 = time.perf_counter()
        e, _, m = R.analyse(x64, n, f0_h[b], SR, HOP, A32)
        took += time.perf_counter() - t0
        noise = 2.0 ** -22 * np.abs(x64).max() * np.random.RandomState(b).standard_normal(n)
        e2, _, m2 = R.analyse(x64 + noise, n, f0_h[b], SR, HOP, A32)
        fig_e = max(fig_e, float(np.abs(np.log(e2[:keep]) - np.log(e[:keep])).max()))
        fig_m = max(fig_m, float(np.abs(m2[:keep] - m[:keep]).max()))
        off_e = max(off_e, float(np.abs(np.log(env_h[b, :keep]) - np.log(e[:keep])).max()))
        off_m = max(off_m, float(np.abs(mc_h[b, :keep] - m[:keep]).max()))
        nf += T
    say("  %-84s %.0f ms for %d frames of %d utterances (%.0f ms for the batch's %d frames at that rate)"
        % ("NumPy float64 replay on the host", took * 1e3, nf, U, took * 1e3 * sum(frames) / nf, sum(frames)))
    say("  conditioning figure (replay under input noise of 2^-22 of the peak): log env %.3e nepers, mc %.3e; device off the replay by "
        "%.3e and %.3e (%.2f x and %.2f x the figure; 8 x is allowed)" % (fig_e, fig_m, off_e, off_m, off_e / fig_e, off_m / fig_m))


say("Spectral envelope and mel-cepstra on the device (csrc/envelope.hip): scripts/prof_envelope.py on one MI355X (torch names it %r), "
    "and the compiler's resource report." % torch.cuda.get_device_name(0))
say("")
say("== python scripts/prof_envelope.py ==")
say("envelope at %d Hz, a hop of %d, fft_size %d, order %d, alpha %g: the F0 of pitch.f0_track; device events around whole warm calls, "
    "median of %d" % (SR, HOP, envelope.fft_size(SR), ORDER, envelope.alpha_for(SR), a.reps))
stft = TacotronSTFT().cuda()
host = np.stack([pitch_ref.voice(N, CFG, 100 + b) for b in range(B)])
run("full length", host, [N] * B, stft)
run("LJS-like ragged lengths", host, [HOP * (n - 1) for n in synth.ljs_like_lengths(B, seed=1234, t_max=N // HOP)[0]], stft)
run("four utterances of 862 / 640 / 410 / 200 frames", host, [HOP * (n - 1) for n in (862, 640, 410, 200)], stft)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
