"""Pitch and pace of audio on the device: what a call costs.  Whole warm calls of prosody.marks and prosody.modify between device
events, median of --reps, at 22.05 kHz and a hop of 256 -- 64 utterances of 220,672 samples, the same batch with LJS-like ragged
lengths, and four utterances of 862 / 640 / 410 / 200 frames -- beside pitch.f0_track on the same audio in the same run, and the
NumPy replay (tests/prosody_ref.py) of some utterances on the host, whose marks and output must equal the device's bit for bit.
The F0 is pitch.f0_track's, the ratio prosody.pitch_ratio's (three semitones up, half the range), the pace 1.1.
Writes --out (profiles/prosody_prof.txt).  --resources: appends the compiler's register / LDS / scratch report of the kernels
to --out instead (needs hipcc, no GPU).
usage: python scripts/prof_prosody.py [--reps R] [--warmup W] [--batch B] [--samples N] [--replay-utterances U] [--out FILE] [--resources]"""
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
ap.add_argument("--replay-utterances", type=int, default=2, help="how many utterances the host replays (its time is scaled to the batch)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prosody_prof.txt"))
ap.add_argument("--resources", action="store_true")
a = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


if a.resources:
    from flowtron_amd import build
    src = os.path.join(build.CSRC, "prosody.hip")
    r = subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-c", src, "-o", os.devnull,
                                                         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    say("")
    say("== python scripts/prof_prosody.py --resources ==")
    say("compiler resource report, csrc/prosody.hip (%s):" % " ".join(build.FLAGS))
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            k = re.search(r"(psola_[a-z]+_k)", text)
            name = k.group(1) if k else text
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
import pitch_ref
import prosody_ref as R
from flowtron_amd import pitch, prosody
from oracle import synth

B, N, SR, HOP = a.batch, a.samples, 22050, 256
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
    say("  %-72s median %.3f ms (min %.3f, max %.3f, %d calls)" % (what, float(np.median(t)), t.min(), t.max(), len(t)))


def run(name, host, ns):
    Bn = len(ns)
    audio = torch.from_numpy(host[:Bn]).cuda()
    n32 = torch.tensor(ns, dtype=torch.int32).cuda()
    frames = torch.tensor([n // HOP + 1 for n in ns]).cuda()
    f0 = pitch.f0_track(audio, ns, SR, HOP)[0]
    ratio = prosody.pitch_ratio(f0, frames, shift_semitones=3.0, range_scale=0.5)
    kw = dict(sampling_rate=SR, hop_length=HOP, pitch_ratio=ratio, pace=1.1)
    m = prosody.marks(audio, n32, f0, **kw)
    out, n_out = prosody.modify(audio, n32, f0, **kw)
    K, J = m.n_analysis.tolist(), m.n_synthesis.tolist()
    say("%s (%d utterances, %d samples in all; %d analysis and %d synthesis marks, at most %d and %d an utterance; %.1f %% of the frames voiced):"
        % (name, Bn, sum(ns), sum(K), sum(J), max(K), max(J), 100.0 * float((f0 > 0).sum()) / float(frames.sum())))
    show("prosody.marks (one launch, a wave per utterance)", timed(lambda: prosody.marks(audio, n32, f0, **kw)))
    show("prosody.modify (two launches: the marks and the overlap-add)", timed(lambda: prosody.modify(audio, n32, f0, **kw)))
    show("pitch.f0_track on the same audio (two launches)", timed(lambda: pitch.f0_track(audio, ns, SR, HOP)))
    U = min(a.replay_utterances, Bn)
    f0_h, ratio_h, out_h = f0.cpu().numpy(), ratio.cpu().numpy(), out.cpu().numpy()
    t0 = time.perf_counter()
    ref = [R.modify(host[b, :ns[b]], f0_h[b, :ns[b] // HOP + 1], float(SR), HOP, ratio_h[b, :ns[b] // HOP + 1], 1.1) for b in range(U)]
    took = time.perf_counter() - t0
    same = all(K[b] == len(w["analysis"]) and J[b] == len(w["synthesis"]) and m.analysis[b, :K[b]].cpu().numpy().tobytes() == w["analysis"].tobytes()
               and m.synthesis[b, :J[b]].cpu().numpy().tobytes() == w["synthesis"].tobytes()
               and m.source[b, :J[b]].cpu().numpy().tobytes() == w["source"].tobytes() and m.half[b, :J[b]].cpu().numpy().tobytes() == w["half"].tobytes()
               and out_h[b, :w["n_out"]].tobytes() == o.tobytes() for b, (o, w) in enumerate(ref))
    share = sum(ns[:U]) / float(sum(ns))
    say("  %-72s %.0f ms for %d utterances (%.0f ms for the %d at that rate); marks and output %s the device's"
        % ("NumPy replay of modify on the host", took * 1e3, U, took * 1e3 / share, Bn, "EQUAL" if same else "DIFFER FROM"))


say("Pitch and pace of audio on the device (csrc/prosody.hip): scripts/prof_prosody.py on one MI355X (torch names it %r), and the "
    "compiler's resource report." % torch.cuda.get_device_name(0))
say("")
say("== python scripts/prof_prosody.py ==")
say("prosody at %d Hz, a hop of %d: the F0 of pitch.f0_track, the ratio of prosody.pitch_ratio (three semitones up, half the range), pace "
    "1.1; device events around whole warm calls, median of %d" % (SR, HOP, a.reps))
host = np.stack([pitch_ref.voice(N, CFG, 100 + b) for b in range(B)])
run("full length", host, [N] * B)
run("LJS-like ragged lengths", host, [HOP * (n - 1) for n in synth.ljs_like_lengths(B, seed=1234, t_max=N // HOP)[0]])
run("four utterances of 862 / 640 / 410 / 200 frames", host, [HOP * (n - 1) for n in (862, 640, 410, 200)])
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
