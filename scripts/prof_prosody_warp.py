"""A pace that varies within the utterance: what a call costs.  Whole warm calls of prosody.warp_marks, prosody.warp and
prosody.time_map_from_path between device events, median of --reps, at 22.05 kHz and a hop of 256 -- 64 utterances of 220,672
samples, the same batch with LJS-like ragged lengths, and four utterances of 862 / 640 / 410 / 200 frames -- beside prosody.marks
and prosody.modify at the constant pace of the same length in the same run, and the NumPy replay (tests/prosody_warp_ref.py) of
some utterances on the host, whose marks and output must equal the device's bit for bit.  The F0 is pitch.f0_track's, the map
1.2 times as long with the pace swinging sinusoidally by a half, the ratio prosody.pitch_ratio's (three semitones up, half the
range) on the input's axis and a contour of the same kind on the output's.
Writes --out (profiles/prosody_warp_prof.txt).  --resources: appends the compiler's register / LDS / scratch report of the
kernels to --out instead (needs hipcc, no GPU).
usage: python scripts/prof_prosody_warp.py [--reps R] [--warmup W] [--batch B] [--samples N] [--replay-utterances U] [--out FILE] [--resources]"""
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
ap.add_argument("--replay-utterances", type=int, default=1, help="how many utterances the host replays")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prosody_warp_prof.txt"))
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
    say("== python scripts/prof_prosody_warp.py --resources ==")
    say("compiler resource report, csrc/prosody.hip (%s):" % " ".join(build.FLAGS))
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            k = re.search(r"(psola_[a-z_]+_k)", text)
            name = k.group(1) if k else text
            row = []
        elif name and re.match(r"(VGPRs|AGPRs|TotalSGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)", text):
            row.append(text)
            if text.startswith("LDS Size"):
                say("  %-20s %s" % (name, "; ".join(row)))
                name = None
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)

import torch
import pitch_ref
import prosody_warp_ref as W
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
    say("  %-84s median %.3f ms (min %.3f, max %.3f, %d calls)" % (what, float(np.median(t)), t.min(), t.max(), len(t)))


def run(name, host, ns):
    Bn = len(ns)
    audio = torch.from_numpy(host[:Bn]).cuda()
    n32 = torch.tensor(ns, dtype=torch.int32).cuda()
    frames = torch.tensor([n // HOP + 1 for n in ns]).cuda()
    f0 = pitch.f0_track(audio, ns, SR, HOP)[0]
    n_out = [n * 6 // 5 for n in ns]
    N_out = max(n_out)
    TM = N_out // HOP + 2
    tm = np.zeros((Bn, TM), np.int64)
    for b, (n, no) in enumerate(zip(ns, n_out)):
        v = np.arange(TM) * HOP / float(no)
        tm[b] = np.rint(np.minimum(n * (v + 0.08 * np.sin(2 * np.pi * v)), n) * 256.0)
    tmap = torch.from_numpy(tm.astype(np.int32)).cuda()
    no32 = torch.tensor(n_out, dtype=torch.int32).cuda()
    r_in = prosody.pitch_ratio(f0, frames, shift_semitones=3.0, range_scale=0.5)
    t_out = torch.arange(N_out // HOP + 1, device="cuda", dtype=torch.float32)
    r_out = torch.exp2(0.25 + 0.2 * torch.sin(t_out / 40.0))[None, :].expand(Bn, -1).contiguous()
    kw_in = dict(sampling_rate=SR, hop_length=HOP, pitch_ratio=r_in, max_out=N_out)
    kw_out = dict(sampling_rate=SR, hop_length=HOP, pitch_ratio=r_out, ratio_axis="output", max_out=N_out)
    kw_old = dict(sampling_rate=SR, hop_length=HOP, pitch_ratio=r_in, pace=1.0 / 1.2)
    m = prosody.warp_marks(audio, n32, f0, tmap, no32, **kw_out)
    out, got_n = prosody.warp(audio, n32, f0, tmap, no32, **kw_out)
    old = prosody.marks(audio, n32, f0, **kw_old)
    K, J, J_old = m.n_analysis.tolist(), m.n_synthesis.tolist(), old.n_synthesis.tolist()
    say("%s (%d utterances, %d samples in, %d out; %d analysis and %d synthesis marks, at most %d and %d an utterance; marks at the "
        "constant pace 1 / 1.2: %d synthesis marks; %.1f %% of the frames voiced):"
        % (name, Bn, sum(ns), sum(n_out), sum(K), sum(J), max(K), max(J), sum(J_old), 100.0 * float((f0 > 0).sum()) / float(frames.sum())))
    show("prosody.warp_marks, ratio on the output's axis (one launch, a wave per utterance)", timed(lambda: prosody.warp_marks(audio, n32, f0, tmap, no32, **kw_out)))
    show("prosody.warp_marks, ratio on the input's axis", timed(lambda: prosody.warp_marks(audio, n32, f0, tmap, no32, **kw_in)))
    show("prosody.marks at the constant pace 1 / 1.2 (one launch, a wave per utterance)", timed(lambda: prosody.marks(audio, n32, f0, **kw_old)))
    show("prosody.warp, ratio on the output's axis (two launches: the marks and the overlap-add)", timed(lambda: prosody.warp(audio, n32, f0, tmap, no32, **kw_out)))
    show("prosody.warp, ratio on the input's axis", timed(lambda: prosody.warp(audio, n32, f0, tmap, no32, **kw_in)))
    show("prosody.modify at the constant pace 1 / 1.2 (two launches)", timed(lambda: prosody.modify(audio, n32, f0, **kw_old)))
    U = min(a.replay_utterances, Bn)
    f0_h, r_h, out_h = f0.cpu().numpy(), r_out.cpu().numpy(), out.cpu().numpy()
    t0 = time.perf_counter()
    ref = [W.warp(host[b, :ns[b]], f0_h[b, :ns[b] // HOP + 1], float(SR), HOP, tm[b], n_out[b], r_h[b], 1) for b in range(U)]
    took = time.perf_counter() - t0
    same = all(K[b] == len(w["analysis"]) and J[b] == len(w["synthesis"]) and m.analysis[b, :K[b]].cpu().numpy().tobytes() == w["analysis"].tobytes()
               and m.synthesis[b, :J[b]].cpu().numpy().tobytes() == w["synthesis"].tobytes()
               and m.source[b, :J[b]].cpu().numpy().tobytes() == w["source"].tobytes() and m.half[b, :J[b]].cpu().numpy().tobytes() == w["half"].tobytes()
               and out_h[b, :w["n_out"]].tobytes() == o.tobytes() for b, (o, w) in enumerate(ref))
    say("  %-84s %.0f ms for %d utterance(s); marks and output %s the device's"
        % ("NumPy replay of warp on the host", took * 1e3, U, "EQUAL" if same else "DIFFER FROM"))


say("A pace that varies within the utterance (csrc/prosody.hip): scripts/prof_prosody_warp.py on one MI355X (torch names it %r), and "
    "the compiler's resource report." % torch.cuda.get_device_name(0))
say("")
say("== python scripts/prof_prosody_warp.py ==")
say("prosody at %d Hz, a hop of %d on both sides: the F0 of pitch.f0_track, a map 1.2 times as long whose pace swings by a half; device "
    "events around whole warm calls, median of %d" % (SR, HOP, a.reps))
host = np.stack([pitch_ref.voice(N, CFG, 100 + b) for b in range(B)])
run("full length", host, [N] * B)
run("LJS-like ragged lengths", host, [HOP * (n - 1) for n in synth.ljs_like_lengths(B, seed=1234, t_max=N // HOP)[0]])
run("four utterances of 862 / 640 / 410 / 200 frames", host, [HOP * (n - 1) for n in (862, 640, 410, 200)])

# a warping path to a map: 64 paths of 1725 cells (863 frames against 863, the staircase of a path at pace 1.2 on a diagonal)
Tp = 863
i = np.arange(2 * Tp - 1) // 2
cells = np.stack([np.minimum(i, Tp - 1), np.minimum(np.arange(2 * Tp - 1) - i, Tp - 1)], 1).astype(np.int32)
path = torch.from_numpy(np.tile(cells[None], (B, 1, 1))).cuda()
plen = torch.full((B,), len(cells), dtype=torch.int32).cuda()
say("a warping path to a time map (%d paths of %d cells, %d map entries each):" % (B, len(cells), Tp + 1))
for w in (0, 4, 32):
    tmap = prosody.time_map_from_path(path, plen, HOP, Tp, smooth=w)
    same = tmap[0].cpu().numpy().tobytes() == W.time_map_from_path(cells, len(cells), HOP, Tp + 1, w).tobytes()
    show("prosody.time_map_from_path, smooth = %d (one launch, a workgroup per path); the replay's bits: %s" % (w, "EQUAL" if same else "DIFFER"),
         timed(lambda: prosody.time_map_from_path(path, plen, HOP, Tp, smooth=w)))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
