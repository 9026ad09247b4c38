"""The encoder's persistent BiLSTM backward on its own: time per launch and per step, the stage stamps of one workgroup, and a dump
of its results for a comparison between two builds.  GPU box:

  python scripts/exp/bilstm_bwd_split_probe.py [--T 157 --B 32 --fmt 1] [--stamps] [--dump FILE.pt] [--compare A.pt B.pt]

--dump writes the forward's outputs, dgx of both directions and a free-running float64 backward (the kernels' operand roundings) on
fixed-seed inputs; --compare reads two such files (two processes, two builds): forward outputs must be torch.equal, dgx is reported
as rel-L2 between the two and of each against the float64 backward."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

H = 256
STAGES = ("poll", "row loads + MFMAs + partial", "barrier + reduce", "cell", "publish + store")


def op16(t, fmt):
    return t.to(torch.float16 if fmt == 2 else torch.bfloat16).double()


def bwd64(dy, w, lens, g, c, fmt, reverse):
    """float64 backward recurrence of one direction from the saved gates / cells, op16 on W_hh and on each step's dgates"""
    T, B = dy.shape[:2]
    W = op16(w, fmt)
    valid = (torch.arange(T, device=dy.device)[:, None] < lens.long()[None, :])
    vm = valid.double()[..., None]
    gd, cd = g.double() * vm, c.double() * vm
    gi, gf, gg, go = gd.chunk(4, -1)
    tc = torch.tanh(cd)
    da = torch.zeros(T, B, 4 * H, dtype=torch.float64, device=dy.device)
    dc_next = torch.zeros(B, H, dtype=torch.float64, device=dy.device)
    f_next, rec = torch.zeros_like(dc_next), torch.zeros_like(dc_next)
    for t in (range(T) if reverse else reversed(range(T))):
        tp = t + 1 if reverse else t - 1                 # the recurrence's previous step
        v = vm[t]
        dh = (dy[t].double() + rec) * v
        dc = (dh * go[t] * (1 - tc[t] ** 2) + f_next * dc_next) * v
        c_prev = cd[tp] * vm[tp] if 0 <= tp < T else torch.zeros_like(dc)
        a = torch.cat([dc * gg[t] * gi[t] * (1 - gi[t]), dc * c_prev * gf[t] * (1 - gf[t]), dc * gi[t] * (1 - gg[t] ** 2),
                       dh * tc[t] * go[t] * (1 - go[t])], -1) * v
        da[t] = a
        # a row that has not started yet (reverse direction, t >= len) passes zeros on: v masks it above
        rec = op16(a, fmt) @ W
        dc_next, f_next = dc, gf[t] * v
    return da


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    for k in ("y", "g0", "g1", "c0", "c1"):
        print("forward %-3s %s" % (k, "equal" if torch.equal(a[k], b[k]) else "DIFFERS max %.3g" % float((a[k] - b[k]).abs().max())))
    for d in range(2):
        k = "d%d" % d
        ab, ar, br = rel(a[k], b[k]), rel(a[k], a["ref" + str(d)]), rel(b[k], b["ref" + str(d)])
        print("dgx dir %d: rel-L2 A vs B %.3e   A vs float64 %.3e   B vs float64 %.3e   (B - A) vs float64 %.3e  %s" % (
            d, ab, ar, br, br - ar, "ok" if br - ar <= ab else "B IS FURTHER FROM float64 THAN THE A-B DISTANCE ALLOWS"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=157)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--fmt", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stamps", action="store_true")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    from flowtron_amd import _lib as L
    T, B, fmt = args.T, args.B, args.fmt
    if (T, B) == (157, 32):
        import bench
        lens = [int(v) for v in bench.synth_batch(B, 1234 + 7)["in_lens"]]
    else:
        lens = [T] + [max(1, T - (3 * i) % T) for i in range(1, B)]
    gen = torch.Generator().manual_seed(5)
    gx = [(torch.randn(T, B, 4 * H, generator=gen) * 0.5).cuda() for _ in range(2)]
    w = [(torch.randn(4 * H, H, generator=gen) / H ** 0.5).cuda() for _ in range(2)]
    dy = (torch.randn(T, B, 2 * H, generator=gen) * 0.1).cuda()
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    f = dict(device="cuda", dtype=torch.float32)
    y = torch.full((T, B, 2 * H), 7.0, **f)
    g = [torch.zeros(T, B, 4 * H, **f) for _ in range(2)]
    c = [torch.zeros(T, B, H, **f) for _ in range(2)]
    d = [torch.full((T, B, 4 * H), 7.0, **f) for _ in range(2)]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = L.lib()
    wk = torch.empty(lib.ft_bilstm_persist_workspace_bytes(B, H), device="cuda", dtype=torch.uint8)
    fw = lambda: L.check(L.op16("ft_bilstm_persist_fwd", fmt)(L.ptr(gx[0]), L.ptr(gx[1]), L.ptr(w[0]), L.ptr(w[1]), L.ptr(lens_t), L.ptr(y), 2 * H,
                                                               L.ptr(g[0]), L.ptr(g[1]), L.ptr(c[0]), L.ptr(c[1]), L.ptr(wk), L.ptr(status), T, B, H, L.stream()), "fwd")
    bw = lambda: L.check(L.op16("ft_bilstm_persist_bwd", fmt)(L.ptr(dy), 2 * H, L.ptr(w[0]), L.ptr(w[1]), L.ptr(lens_t), L.ptr(g[0]), L.ptr(g[1]),
                                                               L.ptr(c[0]), L.ptr(c[1]), L.ptr(d[0]), L.ptr(d[1]), L.ptr(wk), L.ptr(status), T, B, H, L.stream()), "bwd")
    fw(); bw(); torch.cuda.synchronize()
    assert int(status.item()) == 0, "persistent launch did not complete: status %d" % int(status.item())
    for name, fn in (("fwd", fw), ("bwd", bw)):
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts.sort()
        print("%s entry point (memsets + fragment kernel + recurrence), T %d B %d fmt %d: min %.1f us  median %.1f us  (%.2f us per step at the median)" % (
            name, T, B, fmt, ts[0], ts[len(ts) // 2], ts[len(ts) // 2] / T))
    assert int(status.item()) == 0
    if args.stamps:
        assert hasattr(lib, "ft_bilstm_persist_debug_prof"), "this build has no stage stamps"
        buf = torch.zeros(1024 * 4 * 6, dtype=torch.int64, device="cuda")
        L.check(lib.ft_bilstm_persist_debug_prof(L.ptr(buf)), "prof on")
        bw(); torch.cuda.synchronize()
        L.check(lib.ft_bilstm_persist_debug_prof(None), "prof off")
        s = buf.view(1024, 4, 6)[1:max(lens[:4])].double() * 0.01          # 100 MHz ticks -> us; step 0 has no hand-off
        print("stage stamps of the workgroup (XCD 0, slot 0), steps 1 .. %d, us (mean over steps; 10 ns clock):" % (s.shape[0]))
        for wv in range(4):
            ns = 5 if wv == 0 else 3                     # waves 1 .. 3 end their step behind the barrier
            dur = (s[:, wv, 1:ns + 1] - s[:, wv, :ns]).mean(0)
            per = (s[1:, wv, 0] - s[:-1, wv, 0]).mean()
            print("  wave %d: " % wv + "  ".join("%s %.2f" % (n, float(v)) for n, v in zip(STAGES, dur)) + "   | step to step %.2f" % float(per))
    if args.dump:
        ref = [bwd64(dy[..., k * H:(k + 1) * H], w[k], lens_t, g[k], c[k], fmt, bool(k)) for k in range(2)]
        valid = (torch.arange(T, device="cuda")[:, None] < lens_t[None, :])[..., None]
        torch.save({"y": y.cpu(), "g0": (g[0] * valid).cpu(), "g1": (g[1] * valid).cpu(), "c0": (c[0] * valid).cpu(), "c1": (c[1] * valid).cpu(),
                    "d0": d[0].cpu(), "d1": d[1].cpu(), "ref0": ref[0].cpu(), "ref1": ref[1].cpu()}, args.dump)
        print("dumped", args.dump)


if __name__ == "__main__":
    main()
