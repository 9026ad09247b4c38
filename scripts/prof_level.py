"""Endpoints and loudness on the device: what a call costs.  B utterances of up to N samples at 22.05 kHz (frames of 2048 samples
every 512, steps of 2205): active_bounds, loudness, trim and prepare as whole calls, full length and with LJS-like ragged
lengths -- device events around whole warm calls, median of --reps -- beside pitch.f0 on the same audio in the same run, and the
NumPy replay (tests/level_ref.py) of the same audio on the host, whose bounds, gated power and output must equal the device's bit
for bit.  --resources: the compiler's register / LDS / scratch report of the kernels instead (needs hipcc, no GPU).
usage: python scripts/prof_level.py [--reps R] [--warmup W] [--batch B] [--samples N] [--replay-utterances U] [--resources]"""
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
ap.add_argument("--resources", action="store_true")
a = ap.parse_args()

if a.resources:
    from flowtron_amd import build
    src = os.path.join(build.CSRC, "level.hip")
    r = subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-c", src, "-o", os.devnull,
                                                         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    print("compiler resource report, csrc/level.hip (%s):" % " ".join(build.FLAGS))
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            k = re.search(r"(level_[a-z]+_k)(ILi(\d)E)?", text)
            name = (k.group(1) + ("<%s>" % k.group(3) if k.group(3) else "")) if k else text
            row = []
        elif name and re.match(r"(VGPRs|AGPRs|TotalSGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)", text):
            row.append(text)
            if text.startswith("LDS Size"):
                print("  %-20s %s" % (name, "; ".join(row)))
                name = None
    sys.exit(0)

import torch
import level_ref as R
from flowtron_amd import level, pitch
from oracle import synth

B, N, SR = a.batch, a.samples, 22050


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


host = np.stack([R.voice(N, SR, 11025 + 500 * b, N - 8000 - 300 * b, seed=b, amplitude=0.02 + 0.01 * (b % 20)) for b in range(B)])
audio = torch.from_numpy(host).cuda()
ragged = [256 * (n - 1) for n in synth.ljs_like_lengths(B, seed=1234, t_max=N // 256)[0]]
print("level, B %d utterances of up to %d samples at %d Hz (%.1f MB of audio), frames of 2048 every 512, %d chunks of %d samples an "
      "utterance; device events around whole warm calls" % (B, N, SR, B * N * 4 / 1e6, -(-N // level.CHUNK), level.CHUNK))
print("expectation from the arithmetic: the audio is read in a few microseconds; loudness is bound by dependent float64 steps, two "
      "passes of %d per lane and %d carry steps per utterance: tens of microseconds" % (level.CHUNK, -(-N // level.CHUNK)))
for name, ns in (("full length", [N] * B), ("LJS-like ragged lengths", ragged)):
    n32 = torch.tensor(ns, dtype=torch.int32).cuda()
    print("%s (%d samples in all):" % (name, sum(ns)))
    show("level.active_bounds (2 launches)", timed(lambda: level.active_bounds(audio, n32)))
    show("level.loudness (4 launches + torch's log10)", timed(lambda: level.loudness(audio, n32, SR)))
    show("level.trim (3 launches)", timed(lambda: level.trim(audio, n32)))
    show("level.prepare (7 launches + torch's gain arithmetic)", timed(lambda: level.prepare(audio, n32, SR)))
    show("pitch.f0 on the same audio (one launch)", timed(lambda: pitch.f0(audio, ns)))
    out, n_out, info = level.prepare(audio, n32, SR)
    out_h, n_h, s_h, e_h, g_h = out.cpu().numpy(), n_out.tolist(), info.start.tolist(), info.end.tolist(), info.gain.cpu().numpy()
    power_h = level.loudness(audio, n32, SR, start=info.start, end=info.end, return_all=True).power.cpu().numpy()
    U = min(a.replay_utterances, B)
    t0 = time.perf_counter()
    ref = [R.prepare(host[b, :ns[b]], N, SR) for b in range(U)]
    took = time.perf_counter() - t0
    same = all((s_h[b], e_h[b], n_h[b]) == (r["start"], r["end"], r["n_out"]) and power_h[b].tobytes() == np.float64(r["power"]).tobytes()
               and g_h[b].tobytes() == r["gain"].tobytes() and out_h[b].tobytes() == r["out"].tobytes() for b, r in enumerate(ref))
    share = sum(ns[:U]) / float(sum(ns))
    print("  %-72s %.0f ms for %d utterances (%.0f ms for the %d at that rate); bounds, gated power, gain and output %s the device's"
          % ("NumPy replay of prepare on the host", took * 1e3, U, took * 1e3 / share, B, "EQUAL" if same else "DIFFER FROM"))
    lufs_h = info.lufs.cpu().numpy()
    print("  trimmed to %.1f %% of the samples; loudness before %.2f .. %.2f LUFS (%d utterances shorter than a block), gains %.3f .. %.3f"
          % (100.0 * sum(n_h) / sum(ns), np.nanmin(lufs_h), np.nanmax(lufs_h), int(np.isnan(lufs_h).sum()), float(g_h.min()), float(g_h.max())))
