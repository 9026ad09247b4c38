"""Scoring utterances on the device: what a call costs.  score.frame_log_likelihood at B utterances of T frames, M channels and
two flows (log_s as column slices of [T, B, 2M] tensors, the second flow reversed), and score.attention_diagnostics at F flows,
B utterances, T frames and L tokens -- full length, then LJS-like ragged lengths -- device events around whole warm calls,
median of --reps; each next to the NumPy replay (tests/score_ref.py) of the same data on the host, whose results must equal the
device's (the likelihood bit for bit, peaks and counters exactly).
--resources: the compiler's register / LDS / scratch report of the kernels instead (needs hipcc, no GPU).
usage: python scripts/prof_score.py [--reps R] [--warmup W] [--batch B] [--frames T] [--mels M] [--flows F] [--tokens L] [--resources]"""
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
ap.add_argument("--mels", type=int, default=80)
ap.add_argument("--flows", type=int, default=2)
ap.add_argument("--tokens", type=int, default=190)
ap.add_argument("--resources", action="store_true")
a = ap.parse_args()

if a.resources:
    from flowtron_amd import build
    src = os.path.join(build.CSRC, "score.hip")
    r = subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-c", src, "-o", os.devnull,
                                                         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    print("compiler resource report, csrc/score.hip (%s):" % " ".join(build.FLAGS))
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            k = re.search(r"(frame_ll_k|total_ll_k|attn_diag_k)", text)
            name = k.group(1) if k else text
            row = []
        elif name and re.match(r"(VGPRs|AGPRs|TotalSGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)", text):
            row.append(text)
            if text.startswith("LDS Size"):
                print("  %-14s %s" % (name, "; ".join(row)))
                name = None
    sys.exit(0)

import torch
import score_ref as R
from flowtron_amd import score
from oracle import synth

B, T, M, F, Lt = a.batch, a.frames, a.mels, a.flows, a.tokens


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


out_lens, in_lens = synth.ljs_like_lengths(B, seed=1234, t_max=T)
in_lens = [min(l, Lt) for l in in_lens]
g = torch.Generator().manual_seed(0)
z = torch.randn(T, B, M, generator=g).cuda()
wide = [(0.3 * torch.randn(T, B, 2 * M, generator=g)).cuda() for _ in range(2)]
log_s = [w[:, :, M:] for w in wide]
rev = [False, True]
print("score.frame_log_likelihood, B %d, %d frames, %d channels, two flows; device events around whole warm calls" % (B, T, M))
for name, ol in (("full length", [T] * B), ("LJS-like ragged lengths", out_lens)):
    print("%s (mean %.0f frames):" % (name, np.mean(ol)))
    # lengths as device tensors would cost a read-back per call; lists are what a caller holds
    show("frame_log_likelihood (two launches)", timed(lambda: score.frame_log_likelihood(z, log_s, ol, 1.0, rev)))
    got = score.frame_log_likelihood(z, log_s, ol, 1.0, rev)
    zh, lh = z.cpu().numpy(), [x.cpu().numpy() for x in log_s]
    t0 = time.perf_counter()
    rf, rt = R.frame_loglik(zh, lh, rev, ol, 1.0)
    host = time.perf_counter() - t0
    same = got.frame_ll.cpu().numpy().tobytes() == rf.tobytes() and got.total.cpu().numpy().tobytes() == rt.tobytes()
    print("  %-72s %.0f ms for the %d utterances; frame_ll and total %s the device's bit for bit"
          % ("NumPy float64 replay on the host", host * 1e3, B, "EQUAL" if same else "DIFFER FROM"))

attn = torch.softmax(2.0 * torch.randn(F, B, T, Lt, generator=g), 3).cuda()
print("score.attention_diagnostics, F %d, B %d, %d frames x %d tokens (one launch):" % (F, B, T, Lt))
for name, il, ol in (("full length", [Lt] * B, [T] * B), ("LJS-like ragged lengths", in_lens, out_lens)):
    print("%s (mean %.0f frames x %.0f tokens):" % (name, np.mean(ol), np.mean(il)))
    show("attention_diagnostics", timed(lambda: score.attention_diagnostics(attn, il, ol)))
    d = score.attention_diagnostics(attn, il, ol)
    ah = attn.cpu().numpy()
    t0 = time.perf_counter()
    rp, rc, rfs = R.attn_diagnostics(ah, il, ol)
    host = time.perf_counter() - t0
    same = np.array_equal(d.peaks.cpu().numpy(), rp) and all(np.array_equal(getattr(d, k).cpu().numpy(), rc[:, :, i])
                                                              for i, k in enumerate(R.COUNTERS))
    print("  %-72s %.0f ms for the %d maps; peaks and counters %s the device's"
          % ("NumPy replay on the host", host * 1e3, F * B, "EQUAL" if same else "DIFFER FROM"))
