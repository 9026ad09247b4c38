"""Gaussian-mixture prior: what it adds to a training step.  Full-width synthetic 2-flow model at B 32, T 862 (LJS-like lengths),
n_components = 8 -- fixed Gaussians, then learned ones -- against the same step at n_components = 0, all three models in one process,
alternating: forward + FlowtronLoss + backward + RAdam step, device-event time, median of --reps after --warmup.  Then the two
likelihood kernels alone (ops.MixtureNLLFn forward and backward on z [862, 32, 80], C 8; fixed: no parameter gradients, learned:
all of them) and the time pooling of the mel encoder's [862, 32, 512] output.
usage: python scripts/prof_mixture.py [--reps R] [--warmup W] [--mode bf16|f32] [--batch B] [--frames T]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import flowtron
from flowtron_amd import ops
from oracle import synth
from radam import RAdam

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--mode", default="bf16")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--frames", type=int, default=862)
ap.add_argument("--components", type=int, default=8)
a = ap.parse_args()
os.environ["FLOWTRON_MFMA"] = a.mode
B, Cn = a.batch, a.components
base = dict(synth.DEFAULT_MODEL_CONFIG, n_flows=2)
out_lens, in_lens = synth.ljs_like_lengths(B, seed=1234, t_max=a.frames)
batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synth.make_batch(base, out_lens, in_lens, seed=3, with_prior=True).items()}
WAYS = {"n_components 0": dict(n_components=0), "%d fixed" % Cn: dict(n_components=Cn, fixed_gaussian=True, mean_scale=3.0),
        "%d learned" % Cn: dict(n_components=Cn, fixed_gaussian=False)}
runs = {}
for name, extra in WAYS.items():
    cfg = dict(base, **extra)
    m = flowtron.Flowtron(**cfg)
    m.load_state_dict(synth.make_state_dict(cfg, seed=3), strict=False)        # (the mixture's entries keep their initialisation)
    m = m.cuda().train()
    crit = flowtron.FlowtronLoss(1.0, cfg["n_components"] > 1, True, True, 0.01, -8)
    runs[name] = (m, crit, RAdam(m.parameters(), lr=1e-4))


def step(name):
    m, crit, opt = runs[name]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    opt.zero_grad()
    out = m(batch["mel"], batch["speaker_ids"], batch["text"], batch["in_lens"], batch["out_lens"], batch["attn_prior"])
    nll, gl, ctc = crit(out, batch["gate_target"], batch["in_lens"], batch["out_lens"])
    (nll + gl + 0.01 * ctc).sum().backward()
    opt.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return np.array(ts)


for _ in range(a.warmup):
    for name in WAYS:
        step(name)
ms = {name: [] for name in WAYS}
for _ in range(a.reps):
    for name in WAYS:                                            # alternate: drift hits every model alike
        ms[name].append(step(name))
med0 = float(np.median(ms["n_components 0"]))
for name in WAYS:
    t = np.array(ms[name])
    print("%s B=%d T=%d step, %s: median %.2f ms (min %.2f, max %.2f, %d runs), %+.2f ms against n_components 0"
          % (a.mode, B, a.frames, name, float(np.median(t)), t.min(), t.max(), a.reps, float(np.median(t)) - med0), flush=True)

g = torch.Generator().manual_seed(0)
T, M = a.frames, 80
lens = torch.tensor(out_lens, dtype=torch.int32, device="cuda")
z = torch.randn(T, B, M, generator=g).cuda().requires_grad_(True)
coupling = [torch.randn(T, B, 2 * M, generator=g).cuda() * 0.1 for _ in range(2)]
log_s = [c[..., :M].requires_grad_(True) for c in coupling]
prob = torch.softmax(torch.randn(B, Cn, generator=g), 1).cuda()
for name, Bm, grads in (("fixed", 1, False), ("learned", B, True)):
    mean = (torch.randn(Bm, M, Cn, generator=g) * 2).cuda().requires_grad_(grads)
    log_var = (torch.randn(Bm, M, Cn, generator=g) * 0.5).cuda().requires_grad_(grads)
    p = prob.clone().requires_grad_(True)
    t_f = timed(lambda: ops.MixtureNLLFn.apply(z, mean, log_var, p, lens, *log_s), a.reps, a.warmup)
    loss = ops.MixtureNLLFn.apply(z, mean, log_var, p, lens, *log_s)
    t_b = timed(lambda: loss.backward(retain_graph=True), a.reps, a.warmup)
    print("mixture NLL %s, z [%d, %d, %d], C %d: forward median %.1f us (min %.1f), backward median %.1f us (min %.1f) -- whole autograd "
          "calls: launches and their allocations" % (name, T, B, M, Cn, np.median(t_f), t_f.min(), np.median(t_b), t_b.min()), flush=True)
h = torch.randn(T, B, 512, generator=g).cuda().requires_grad_(True)
t_f = timed(lambda: ops.TimePoolFn.apply(h, lens), a.reps, a.warmup)
y = ops.TimePoolFn.apply(h, lens)
dy = torch.randn_like(y)
t_b = timed(lambda: y.backward(dy, retain_graph=True), a.reps, a.warmup)
print("time pool [%d, %d, 512]: forward median %.1f us, backward median %.1f us" % (T, B, np.median(t_f), np.median(t_b)), flush=True)
