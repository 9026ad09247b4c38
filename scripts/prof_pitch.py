"""F0 tracking on the device: what a call costs.  B utterances of up to N samples at the default settings (22.05 kHz, hop 256,
window 1024, lags 55 .. 368): the whole pitch.f0 call (one launch), full length and with LJS-like ragged lengths, and
metrics.f0_distortion along full-length paths -- device events around whole warm calls, median of --reps; the NumPy float32
replay (tests/pitch_ref.py) of the same audio on the host, whose F0 and aperiodicity must equal the device's bit for bit.
--resources: the compiler's register / LDS / scratch report of the two kernels instead (needs hipcc, no GPU).
usage: python scripts/prof_pitch.py [--reps R] [--warmup W] [--batch B] [--frames T] [--replay-utterances U] [--resources]"""
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
            k = re.search(r"(yin_k|f0_path_stats_k)", text)
            name = k.group(1) if k else text
            row = []
        elif name and re.match(r"(VGPRs|AGPRs|TotalSGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)", text):
            row.append(text)
            if text.startswith("LDS Size"):
                print("  %-20s %s" % (name, "; ".join(row)))
                name = None
    print("  (yin_k's LDS is dynamic: per frame of the workgroup the window, W + 4 ceil((tau_max + 2) / 4) + 8 floats, and two lag arrays)")
    sys.exit(0)

import torch
import pitch_ref as R
from flowtron_amd import metrics, pitch
from oracle import synth

B, T = a.batch, a.frames
cfg = R.DEFAULT
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


host = np.stack([R.voice(N, cfg, b) for b in range(B)])
audio = torch.from_numpy(host).cuda()
ragged = [hop * (n - 1) for n in synth.ljs_like_lengths(B, seed=1234, t_max=T)[0]]
lags = cfg["tau_max"] + 2
print("YIN, B %d utterances of up to %d samples (%d frames), hop %d, window %d, lags %d .. %d; device events around whole warm calls"
      % (B, N, N // hop + 1, hop, cfg["W"], cfg["tau_min"], cfg["tau_max"]))
for name, ns in (("full length", [N] * B), ("LJS-like ragged lengths", ragged)):
    frames = sum(n // hop + 1 for n in ns)
    ops = 3.0 * frames * lags * cfg["W"]
    print("%s (%d frames in all, %.1f G fp32 operations in the difference function):" % (name, frames, ops / 1e9))
    t = timed(lambda: pitch.f0(audio, ns))
    show("pitch.f0 (one launch)", t)
    print("  %-72s %.1f T fp32 operations per second" % ("", ops / (float(np.median(t)) * 1e-3) / 1e12))
    f0, apd = pitch.f0(audio, ns)
    f0_h, ap_h = f0.cpu().numpy(), apd.cpu().numpy()
    U = min(a.replay_utterances, B)
    t0 = time.perf_counter()
    ref = [R.yin(host[b, :ns[b]], cfg, np.float32) for b in range(U)]
    took = time.perf_counter() - t0
    same = all(f0_h[b, :len(r[0])].tobytes() == r[0].tobytes() and ap_h[b, :len(r[1])].tobytes() == r[1].tobytes() for b, r in enumerate(ref))
    share = sum(ns[:U]) / float(sum(ns))
    print("  %-72s %.0f ms for %d utterances (%.0f ms for the %d at that rate); F0 and aperiodicity %s the device's"
          % ("NumPy float32 replay on the host", took * 1e3, U, took * 1e3 / share, B, "EQUAL" if same else "DIFFER FROM"))
    n_voiced, mean, std = pitch.f0_statistics(f0, [n // hop + 1 for n in ns])
    print("  voiced frames %d of %d, mean spread %.2f semitones" % (int(n_voiced.sum()), frames, float(std[~torch.isnan(std)].mean())))

fr = N // hop + 1
f0_a, _ = pitch.f0(audio)
f0_b = f0_a.flip(0).contiguous()
path = torch.tensor([[i, 0] for i in range(fr)] + [[fr - 1, j] for j in range(1, fr)], dtype=torch.int32).cuda()[None].expand(B, -1, -1).contiguous()
plen = torch.full((B,), 2 * fr - 1, dtype=torch.int32).cuda()
print("f0_distortion, B %d pairs, paths of %d cells:" % (B, 2 * fr - 1))
show("metrics.f0_distortion (one launch + the formula)", timed(lambda: metrics.f0_distortion(f0_a, f0_b, path, plen)))
