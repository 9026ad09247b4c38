"""Probabilistic YIN on the device: what a call costs.  B utterances of up to N samples at the default settings (22.05 kHz, hop 256,
window 1024, lags 55 .. 368, 329 pitch bins, a band of 50), full length and with LJS-like ragged lengths: the whole
pitch.f0_candidates call (one launch), the whole pitch.f0_track call (two launches) and, in the same run as the yardstick,
pitch.f0 (plain YIN: the same difference function) -- device events around whole warm calls, median of --reps; the NumPy
float32 replay (tests/pyin_ref.py) of a few utterances on the host, whose results must equal the device's bit for bit.
--resources: the compiler's register / LDS / scratch report of the two kernels instead (needs hipcc, no GPU).
usage: python scripts/prof_pitch_track.py [--reps R] [--warmup W] [--batch B] [--frames T] [--replay-utterances U] [--resources]"""
import argparse, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--frames", type=int, default=862)
ap.add_argument("--replay-utterances", type=int, default=4, help="how many utterances the host replays (its time is scaled to the batch)")
ap.add_argument("--resources", action="store_true")
a = ap.parse_args()

if a.resources:
    from flowtron_amd import build
    src = os.path.join(build.CSRC, "pitch.hip")
    r = subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-c", src, "-o", os.devnull,
                                                         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    print("compiler resource report, csrc/pitch.hip (%s):" % " ".join(build.FLAGS))
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            k = re.search(r"(pyin_candidates_k|pyin_viterbi_k|yin_k)", text)
            name = k.group(1) if k else None
            row = []
        elif name and re.match(r"(VGPRs|AGPRs|TotalSGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)", text):
            row.append(text)
            if text.startswith("LDS Size"):
                print("  %-20s %s" % (name, "; ".join(row)))
                name = None
    print("  (LDS is dynamic: pyin_candidates_k has yin_k's layout; pyin_viterbi_k holds 4 rows of roundup(n_bins + 2 band, 64) + 32 floats and 176 more)")
    sys.exit(0)

import torch
import pitch_ref as R
import pyin_ref as P
from flowtron_amd import pitch
from oracle import synth

B, T = a.batch, a.frames
cfg = P.config("default")
hop = cfg["hop"]
N = hop * T                                       # 862 frames: 220 672 samples


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
    print("  %-72s median %.3f ms (min %.3f, max %.3f, %d calls)" % (what, float(np.median(t)), t.min(), t.max(), len(t)), flush=True)
    return float(np.median(t))


host = np.stack([R.voice(N, cfg, b) for b in range(B)])
audio = torch.from_numpy(host).cuda()
ragged = [hop * (n - 1) for n in synth.ljs_like_lengths(B, seed=1234, t_max=T)[0]]
print("pYIN, B %d utterances of up to %d samples (%d frames), hop %d, window %d, lags %d .. %d, %d bins, band %d; device events around whole warm calls"
      % (B, N, N // hop + 1, hop, cfg["W"], cfg["tau_min"], cfg["tau_max"], P.n_bins(cfg), P.band(cfg)))
for name, ns in (("full length", [N] * B), ("LJS-like ragged lengths", ragged)):
    frames = sum(n // hop + 1 for n in ns)
    print("%s (%d frames in all, the longest utterance %d):" % (name, frames, max(n // hop + 1 for n in ns)))
    t_yin = show("pitch.f0 (plain YIN, one launch)", timed(lambda: pitch.f0(audio, ns)))
    t_cand = show("pitch.f0_candidates (one launch)", timed(lambda: pitch.f0_candidates(audio, ns)))
    t_track = show("pitch.f0_track (two launches)", timed(lambda: pitch.f0_track(audio, ns)))
    print("  %-72s candidates %.2f x pitch.f0, track %.2f x pitch.f0; the path search alone %.3f ms"
          % ("", t_cand / t_yin, t_track / t_yin, t_track - t_cand))
    prob, freq = pitch.f0_candidates(audio, ns)
    f0, voiced = pitch.f0_track(audio, ns)
    got = dict(prob=prob.cpu().numpy(), freq=freq.cpu().numpy(), f0=f0.cpu().numpy(), voiced=voiced.cpu().numpy())
    U = min(a.replay_utterances, B)
    t0 = time.perf_counter()
    ref = [P.track(host[b, :ns[b]], cfg, np.float32) for b in range(U)]
    took = time.perf_counter() - t0
    same = all(got[k][b, :len(r["f0"])].tobytes() == r[k].tobytes() for b, r in enumerate(ref) for k in got)
    share = sum(ns[:U]) / float(sum(ns))
    print("  %-72s %.0f ms for %d utterances (%.0f ms for the %d at that rate); candidates, F0 and voiced mass %s the device's"
          % ("NumPy float32 replay on the host", took * 1e3, U, took * 1e3 / share, B, "EQUAL" if same else "DIFFER FROM"))
    plain = pitch.f0(audio, ns)[0]
    lens = [n // hop + 1 for n in ns]
    print("  voiced frames: tracker %d, plain YIN %d of %d" % (int(pitch.f0_statistics(f0, lens)[0].sum()), int(pitch.f0_statistics(plain, lens)[0].sum()), frames))

one = audio[:1]
print("one utterance alone (%d frames: one workgroup walks the path):" % (N // hop + 1))
t_c1 = show("pitch.f0_candidates", timed(lambda: pitch.f0_candidates(one)))
t_t1 = show("pitch.f0_track", timed(lambda: pitch.f0_track(one)))
print("  %-72s %.2f us per frame step of the path" % ("", (t_t1 - t_c1) * 1e3 / (N // hop + 1)))
