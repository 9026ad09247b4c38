"""Decode along given alignments: Flowtron.infer_aligned(persistent=True) (one dec_persist_batch_k<F32, true> launch per flow and
group of up to ft_decode_batch_max() utterances, csrc/decode_forced.hip) against (a) infer_aligned(persistent=False), the
utterance-by-utterance loop over the staged forced-decode chain, and (c) the free-running Flowtron.infer of the same batch (the
batched persistent launch; B = 1: dec_persist_k), alternating in one process.
Full-width synthetic 2-flow model, L 150, N 400, ungated, hard rows (N / L frames per token), B = 1, 2, 4, 8, fp32 weights and bf16
weight images: device-event time of whole warm calls, median and spread; us per frame and flow.  --stages: per-stage times inside
the forced launch at B = 1 and 4 from the ft_decode_debug_prof stamps of workgroup 0 (the last flow's launch; medians over the
frames), beside the free-running launch's.
usage: python scripts/prof_decode_aligned.py [--reps R] [--warmup W] [--modes f32,bf16] [--stages] [--batches 1,2,4,8]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import flowtron
from flowtron_amd import align
from oracle import synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--frames", type=int, default=400)
ap.add_argument("--text", type=int, default=150)
ap.add_argument("--modes", default="f32,bf16")
ap.add_argument("--batches", default="1,2,4,8")
ap.add_argument("--stages", action="store_true")
a = ap.parse_args()
cfg = dict(synth.DEFAULT_MODEL_CONFIG, n_text=60, n_flows=2)
m = flowtron.Flowtron(**cfg)
m.load_state_dict(synth.make_state_dict(cfg, seed=17))
m = m.cuda().eval()
g = torch.Generator().manual_seed(0)
Bmax = max(int(b) for b in a.batches.split(","))
residual = (torch.randn(Bmax, 80, a.frames, generator=g) * 0.5).cuda()
text = torch.randint(1, 60, (Bmax, a.text), generator=g).cuda()
spk = torch.zeros(Bmax, dtype=torch.long).cuda()
dur = torch.full((Bmax, a.text), a.frames // a.text, dtype=torch.int32)
dur[:, : a.frames - a.text * (a.frames // a.text)] += 1                        # every utterance: exactly a.frames frames
rows = align.durations_to_alignment(dur.cuda(), [a.text] * Bmax)                # [B, N, L] hard rows, natural time
assert tuple(rows.shape) == (Bmax, a.frames, a.text)
WAYS = ("aligned, staged loop", "aligned, persistent", "free-running infer")


def run(B, way):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if way == WAYS[2]:
        m.infer(residual[:B], spk[:B], text[:B], gate_threshold=1.0)
    else:
        m.infer_aligned(residual[:B], spk[:B], text[:B], rows[:B], persistent=(way == WAYS[1]))
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for mode in a.modes.split(","):
    os.environ["FLOWTRON_MFMA"] = mode
    for B in (int(b) for b in a.batches.split(",")):
        for _ in range(a.warmup):
            for w in WAYS:
                run(B, w)
        ms = {w: [] for w in WAYS}
        for _ in range(a.reps):
            for w in WAYS:                                       # alternate: drift hits every way alike
                ms[w].append(run(B, w))
        for w in WAYS:
            t = np.array(ms[w])
            med = float(np.median(t))
            print("%s B=%d %s: median %.2f ms (min %.2f, max %.2f, %d runs), %.1f us per frame and flow, %.0f utterance-frames/s"
                  % (mode, B, w, med, t.min(), t.max(), a.reps, med * 1e3 / (a.frames * cfg["n_flows"]), B * a.frames / (med * 1e-3)),
                  flush=True)

if a.stages:
    # stamps k = 0..10 (decode_batch_k.h stamp()): 0 frame start, 1 after the o gather, 2 after S1's compute, 3 after the h_att
    # gather, 4 / 5 after the q / scores gathers (forced: no such hops -- 4 with 3, 5 behind the row's copy into LDS), 6..10 after the
    # gathers of ctx, h0, h1, u1, u2; a stage's compute is the gap from its gather to the next stamp
    from flowtron_amd import _lib as L
    buf = torch.zeros(512 * 12, dtype=torch.int64, device="cuda")
    L.check(L.lib().ft_decode_debug_prof(L.ptr(buf)), "ft_decode_debug_prof")
    names = ["o gather", "S1 coupling + attention LSTM", "h_att gather", "S2 query + q gather | forced: -", "S3a scores + scores gather | forced: row -> LDS",
             "S3b (softmax) context + ctx gather", "S4 gate/LSTM0 + h0 gather", "S5 LSTM1 + h1 gather", "S6 dense0 + u1 gather",
             "S7 dense1 + u2 gather", "S8 conv -> next frame"]
    try:
        for mode in a.modes.split(","):
            os.environ["FLOWTRON_MFMA"] = mode
            for B in (1, 4):
                for w in WAYS[1:]:
                    run(B, w)
                    buf.zero_()
                    run(B, w)
                    st = buf.reshape(512, 12)[: min(a.frames, 512)].cpu().numpy().astype(np.float64) * 10.0 / 1e3   # 100 MHz -> us
                    f = slice(4, st.shape[0] - 4)
                    frame = np.median(st[f.start + 1:f.stop + 1, 0] - st[f, 0])
                    d = {k: np.median(st[f, k + 1] - st[f, k]) for k in range(10)}
                    d[10] = np.median(st[f.start + 1:f.stop + 1, 0] - st[f, 10])
                    print("%s B=%d %s, stage stamps (us, median over %d frames): frame %.2f | " % (mode, B, w, f.stop - f.start, frame) +
                          ", ".join("%s %.2f" % (names[k], d[k]) for k in range(11)), flush=True)
    finally:
        L.lib().ft_decode_debug_prof(None)
