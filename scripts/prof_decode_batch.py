"""Batched persistent decode (Flowtron.infer, B > 1: one dec_persist_batch_k launch per flow and group of up to
ft_decode_batch_max() utterances) against the utterance-by-utterance loop (FLOWTRON_DECODE_BATCH=0), alternating in one process.
Full-width synthetic 2-flow model, L 150, N 400, ungated, B = 1, 2, 4, 8, fp32 weights and bf16 weight images: device-event time of whole
warm infer calls, median and spread; us per frame and flow, utterance-frames/s.  --stages: per-stage times inside the launch at B = 1 and 4 from the ft_decode_debug_prof stamps of workgroup 0 (the last flow's launch;
medians over the frames).  --text-lens 40,80,150,300: sentences of different lengths instead, B = their number, three ways
alternating: (a) the ragged batch (in_lens: a key count per utterance), (b) the loop over the trimmed utterances
(FLOWTRON_DECODE_BATCH=0, same in_lens), (c) the same batch unragged at L = the longest (no in_lens).  Kernel times: a separate
`rocprofv3 --kernel-trace --stats -- python scripts/prof_decode_batch.py --reps 1 --warmup 1` run.
usage: python scripts/prof_decode_batch.py [--reps R] [--warmup W] [--modes f32,bf16] [--stages] [--batches 1,2,4,8]
                                           [--text-lens 40,80,150,300]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import flowtron
from oracle import synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--frames", type=int, default=400)
ap.add_argument("--text", type=int, default=150)
ap.add_argument("--modes", default="f32,bf16")
ap.add_argument("--batches", default="1,2,4,8")
ap.add_argument("--stages", action="store_true")
ap.add_argument("--text-lens", default="")
a = ap.parse_args()
text_lens = [int(x) for x in a.text_lens.split(",")] if a.text_lens else []
if text_lens:
    a.batches, a.text = str(len(text_lens)), max(text_lens)
cfg = dict(synth.DEFAULT_MODEL_CONFIG, n_text=60, n_flows=2)
m = flowtron.Flowtron(**cfg)
m.load_state_dict(synth.make_state_dict(cfg, seed=17))
m = m.cuda().eval()
g = torch.Generator().manual_seed(0)
Bmax = max(int(b) for b in a.batches.split(","))
residual = (torch.randn(Bmax, 80, a.frames, generator=g) * 0.5).cuda()
text = torch.randint(1, 60, (Bmax, a.text), generator=g).cuda()
spk = torch.zeros(Bmax, dtype=torch.long).cuda()


def run(B, batched, in_lens=None):
    os.environ["FLOWTRON_DECODE_BATCH"] = "1" if batched else "0"
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    m.infer(residual[:B], spk[:B], text[:B], gate_threshold=1.0, in_lens=in_lens)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


if text_lens:
    B = len(text_lens)
    ways = {"ragged batch": (True, text_lens), "loop over trimmed": (False, text_lens), "unragged batch at L %d" % a.text: (True, None)}
    for mode in a.modes.split(","):
        os.environ["FLOWTRON_MFMA"] = mode
        for _ in range(a.warmup):
            for w in ways.values():
                run(B, *w)
        ms = {k: [] for k in ways}
        for _ in range(a.reps):
            for k, w in ways.items():                            # alternate: drift hits every way alike
                ms[k].append(run(B, *w))
        for k in ways:
            t = np.array(ms[k])
            med = float(np.median(t))
            print("%s B=%d text %s %s: infer median %.2f ms (min %.2f, max %.2f, %d runs), %.1f us per frame and flow"
                  % (mode, B, a.text_lens, k, med, t.min(), t.max(), a.reps, med * 1e3 / (a.frames * cfg["n_flows"])), flush=True)
    sys.exit(0)

for mode in a.modes.split(","):
    os.environ["FLOWTRON_MFMA"] = mode
    for B in (int(b) for b in a.batches.split(",")):
        paths = (True, False) if B > 1 else (False,)
        for _ in range(a.warmup):
            for p in paths:
                run(B, p)
        ms = {p: [] for p in paths}
        for _ in range(a.reps):
            for p in paths:                                      # alternate: drift hits both paths alike
                ms[p].append(run(B, p))
        for p in paths:
            t = np.array(ms[p])
            med = float(np.median(t))
            us = med * 1e3 / (a.frames * cfg["n_flows"])
            print("%s B=%d %s: infer median %.2f ms (min %.2f, max %.2f, %d runs), %.1f us per frame and flow, %.0f utterance-frames/s"
                  % (mode, B, "batched" if p else ("single" if B == 1 else "loop"), med, t.min(), t.max(), a.reps, us,
                     B * a.frames / (med * 1e-3)), flush=True)


if a.stages:
    # stamps k = 0..10 (decode_batch.hip / decode.hip stamp()): 0 frame start, 1 after the o gather, 2 after S1's compute, 3..10 after
    # the gathers of h_att, q, scores, ctx, h0, h1, u1, u2; a stage's compute is the gap from its gather to the next stamp
    from flowtron_amd import _lib as L
    buf = torch.zeros(512 * 12, dtype=torch.int64, device="cuda")
    L.check(L.lib().ft_decode_debug_prof(L.ptr(buf)), "ft_decode_debug_prof")
    try:
        for mode in a.modes.split(","):
            os.environ["FLOWTRON_MFMA"] = mode
            for B in (1, 4):
                run(B, B > 1)
                buf.zero_()
                run(B, B > 1)
                st = buf.reshape(512, 12)[: min(a.frames, 512)].cpu().numpy().astype(np.float64) * 10.0 / 1e3   # 100 MHz -> us
                f = slice(4, st.shape[0] - 4)
                frame = np.median(st[f.start + 1:f.stop + 1, 0] - st[f, 0])
                # intervals between consecutive stamps (the compute after gather k runs into the wait of gather k + 1)
                d = {k: np.median(st[f, k + 1] - st[f, k]) for k in range(10)}
                d[10] = np.median(st[f.start + 1:f.stop + 1, 0] - st[f, 10])
                names = ["o gather", "S1 coupling + attention LSTM", "h_att gather", "S2 query + q gather", "S3a scores + scores gather",
                         "S3b softmax/context + ctx gather", "S4 gate/LSTM0 + h0 gather", "S5 LSTM1 + h1 gather", "S6 dense0 + u1 gather",
                         "S7 dense1 + u2 gather", "S8 conv -> next frame"]
                print("%s B=%d stage stamps (us, median over %d frames): frame %.2f | " % (mode, B, f.stop - f.start, frame) +
                      ", ".join("%s %.2f" % (names[k], d[k]) for k in range(11)), flush=True)
    finally:
        L.lib().ft_decode_debug_prof(None)
