"""MCD-DTW on the device: what a call costs.  B pairs of log-mel-like utterances of up to T frames, K cepstra: the whole
metrics.mel_cepstral_distortion call (two cepstra launches, one warp launch, the dB formula), the warp alone on ready cepstra
and the cepstra alone -- full length, then LJS-like ragged lengths -- device events around whole warm calls, median of --reps;
the NumPy float32 replay (tests/dtw_ref.py) of the same pairs on the host, whose costs and path lengths must equal the
device's bit for bit; and align.monotonic_alignment at the same B and T (L tokens) in the same run.
--resources: the compiler's register / LDS / scratch report of the warp and cepstra kernels instead (needs hipcc, no GPU).
usage: python scripts/prof_mcd.py [--reps R] [--warmup W] [--batch B] [--frames T] [--coeffs K] [--tokens L] [--resources]"""
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
ap.add_argument("--coeffs", type=int, default=13)
ap.add_argument("--tokens", type=int, default=190)
ap.add_argument("--resources", action="store_true")
a = ap.parse_args()

if a.resources:
    from flowtron_amd import build
    src = os.path.join(build.CSRC, "dtw.hip")
    r = subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-c", src, "-o", os.devnull,
                                                         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    print("compiler resource report, csrc/dtw.hip (%s):" % " ".join(build.FLAGS))
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            k = re.search(r"(mel_cepstra_k|dtw_k)ILi(\d+)E", text)
            name = "%s<%s>" % (k.group(1), k.group(2)) if k else text
            row = []
        elif name and re.match(r"(VGPRs|AGPRs|TotalSGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)", text):
            row.append(text)
            if text.startswith("LDS Size"):
                print("  %-20s %s" % (name, "; ".join(row)))
                name = None
    sys.exit(0)

import torch
import dtw_ref as R
from flowtron_amd import align, metrics
from oracle import synth

B, T, K = a.batch, a.frames, a.coeffs


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


mel_a = torch.from_numpy(np.stack([R.log_mel(80, T, 2 * b) for b in range(B)])).cuda()
mel_b = torch.from_numpy(np.stack([R.log_mel(80, T, 2 * b + 1) for b in range(B)])).cuda()
ragged_a = synth.ljs_like_lengths(B, seed=1234, t_max=T)[0]
ragged_b = np.random.RandomState(5).permutation(synth.ljs_like_lengths(B, seed=4321, t_max=T)[0]).tolist()
print("MCD-DTW, B %d pairs, up to %d x %d frames, 80 mel channels, K %d; device events around whole warm calls" % (B, T, T, K))
for name, al, bl in (("full length", [T] * B, [T] * B), ("LJS-like ragged lengths", ragged_a, ragged_b)):
    print("%s (mean %.0f x %.0f frames):" % (name, np.mean(al), np.mean(bl)))
    # lengths as device tensors would cost a read-back per call; lists are what a caller holds after infer
    show("mel_cepstral_distortion (2 cepstra + warp + formula)", timed(lambda: metrics.mel_cepstral_distortion(mel_a, al, mel_b, bl, n_coeffs=K)))
    ca, cb = metrics.mel_cepstra(mel_a, al, K), metrics.mel_cepstra(mel_b, bl, K)
    show("mel_cepstra of one side", timed(lambda: metrics.mel_cepstra(mel_a, al, K)))
    show("dtw on ready cepstra (one launch)", timed(lambda: metrics.dtw(ca, cb, al, bl)))
    show("dtw on the first cepstrum alone (K 1: the steps without the distances)", timed(lambda: metrics.dtw(ca[:, :, :1], cb[:, :, :1], al, bl)))
    show("dtw, diagonal=True (equal lengths: the first side's)", timed(lambda: metrics.dtw(ca, cb, al, al, diagonal=True)))
    cost, path, path_len = metrics.dtw(ca, cb, al, bl)
    cost, path_len, ca_h, cb_h = cost.cpu().numpy(), path_len.cpu().numpy(), ca.cpu().numpy(), cb.cpu().numpy()
    t0 = time.perf_counter()
    ref = [R.replay(ca_h[b, :al[b]], cb_h[b, :bl[b]], np.float32) for b in range(B)]
    host = time.perf_counter() - t0
    same = all(np.float32(c).tobytes() == cost[b:b + 1].tobytes() and len(p) == path_len[b] for b, (c, p) in enumerate(ref))
    print("  %-72s %.0f ms for the %d pairs; costs and path lengths %s the device's" % ("NumPy float32 replay on the host", host * 1e3, B, "EQUAL" if same else "DIFFER FROM"))
    steps = max(x + y - 1 for x, y in zip(al, bl))
    t = float(np.median(timed(lambda: metrics.dtw(ca, cb, al, bl))))
    print("  longest pair: %d dependent anti-diagonal steps, %.0f ns per step of the whole launch" % (steps, t * 1e6 / steps))

Lt = a.tokens
out_lens, in_lens = synth.ljs_like_lengths(B, seed=1234, t_max=T)
logp = torch.randn(B, T, Lt, generator=torch.Generator().manual_seed(0)).cuda()
print("align.monotonic_alignment, B %d, %d frames x %d tokens, in the same run:" % (B, T, Lt))
show("full length", timed(lambda: align.monotonic_alignment(logp, [Lt] * B, [T] * B)))
show("LJS-like ragged lengths", timed(lambda: align.monotonic_alignment(logp, [min(l, Lt) for l in in_lens], out_lens)))
