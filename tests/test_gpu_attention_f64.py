"""(-m gpu) ft_attention_fwd / _bwd and ft_attn_ctc_* against float64 (tests/attn_ref64.py), element by element, on every data-chosen path.

Every output element is compared with its float64 reference and must stay within its bound (attn_ref64's docstrings derive each one);
each case prints its largest error-to-bound ratio.  Each case also asserts, from its own inputs and by the kernel's own rule, that the
path it names is taken.  Sensitivity: each family compares the kernel with the float64 reference of a slightly WRONG operation
under the same bound, and that comparison must fail by at least SHARP."""
import math

import pytest
import torch

import attn_ref64 as R

pytestmark = pytest.mark.gpu
SHARP = 10.0
C2F = torch.tensor(R.C2, dtype=torch.float32)


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.lib()
    return L, ops


def ratio(got, ref, bound, mask=None):
    """max |got - ref| / bound; where the bound is 0 the kernel must be exact (else inf)"""
    err = (got.double() - ref.double()).abs()
    if mask is not None:
        err, bound = err[mask], bound[mask]
    if err.numel() == 0:
        return 0.0
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max())


def amax(t):
    """max |t|, 0 for an empty selection"""
    return float(t.abs().max()) if t.numel() else 0.0


def ptr(t):
    return None if t is None else t.data_ptr()


def run_attention(L, Q, K, v, lens, prior, temp, dattn, dlp):
    """both C entries: the forward, then the backward fed the forward's own attn / p_save"""
    T, B, A = Q.shape
    Lk = K.shape[0]
    attn = torch.empty(B, T, Lk, device="cuda")
    logprob, p_save = torch.empty_like(attn), (torch.empty_like(attn) if prior is not None else None)
    L.check(L.lib().ft_attention_fwd(ptr(Q), ptr(K), ptr(v), ptr(lens), ptr(prior), ptr(attn), ptr(logprob), ptr(p_save), T, B, Lk, A,
                                     float(temp), L.stream()), "ft_attention_fwd")
    de, dQ, dK, dv = torch.empty_like(attn), torch.empty_like(Q), torch.empty_like(K), torch.zeros(A, device="cuda")
    L.check(L.lib().ft_attention_bwd(ptr(Q), ptr(K), ptr(v), ptr(lens), ptr(prior), ptr(attn), ptr(p_save), ptr(dattn), ptr(dlp),
                                     ptr(de), ptr(dQ), ptr(dK), ptr(dv), T, B, Lk, A, float(temp), L.stream()), "ft_attention_bwd")
    torch.cuda.synchronize()
    return dict(attn=attn, logprob=logprob, p_save=p_save, de=de, dQ=dQ, dK=dK, dv=dv)


def dqdk_waves(A):
    """the launcher's wave count per dQ/dK workgroup (attention.hip ft_attention_bwd) and whether the last workgroup has idle waves"""
    nchunk = -(-A // 64)
    nw = nchunk if nchunk < 4 else 4
    if nchunk > 4:
        nw = 4 if nchunk % 4 == 0 else 3 if nchunk % 3 == 0 else 2 if nchunk % 2 == 0 else 4
    return nw, nchunk % nw != 0


def make_attention(T, B, Lk, A, seed, prior=True, scale=0.7, vscale=0.3, lens=None):
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn(T, B, A, generator=g) * scale
    K = torch.randn(Lk, B, A, generator=g) * scale
    v = torch.randn(A, generator=g) * vscale
    if lens is None:
        lens = torch.randint(max(1, Lk // 2), Lk + 1, (B,), generator=g)
        lens[0] = Lk
    pr = None
    if prior:
        pr = torch.rand(B, T, Lk, generator=g) ** 3
        pr[:, :, ::7] = 0.0                                                    # exact zeros in the prior
    valid = (torch.arange(Lk)[None, :] < lens[:, None])[:, None, :]
    dattn = torch.randn(B, T, Lk, generator=g) * valid
    dlp = torch.randn(B, T, Lk, generator=g) * 0.1 * valid
    return dict(Q=Q, K=K, v=v, lens=lens.int(), prior=pr, dattn=dattn, dlp=dlp)


def check_attention(env, c, temp, name, sens=()):
    """runs the case, compares every output with its bound; returns the ratios and asserts them.  sens: names of sensitivity checks"""
    L, ops = env
    d = {k: (t.cuda().contiguous() if torch.is_tensor(t) else t) for k, t in c.items()}
    out = run_attention(L, d["Q"], d["K"], d["v"], d["lens"], d["prior"], temp, d["dattn"], d["dlp"])
    for k in ("attn", "logprob", "de", "dQ", "dK", "dv"):
        assert torch.isfinite(out[k]).all(), (name, k)
    ref = R.attention_fwd(d["Q"], d["K"], d["v"], d["lens"], d["prior"], temp)
    r = dict(attn=ratio(out["attn"], ref["attn"], R.bound_attn(ref)), logprob=ratio(out["logprob"], ref["logprob"], R.bound_logprob(ref)))
    if d["prior"] is not None:
        r["p"] = ratio(out["p_save"], ref["p"], R.bound_p(ref))
    de_ref, de_err = R.attention_de(out["attn"], out["p_save"], d["dattn"], d["dlp"], d["lens"], temp, prior=d["prior"] is not None)
    r["de"] = ratio(out["de"], de_ref, de_err)
    gr = R.attention_grads(d["Q"], d["K"], d["v"], d["lens"], out["de"])
    for k in ("dQ", "dK", "dv"):
        r[k] = ratio(out[k], gr[k], gr[k + "_err"])
    valid = ref["valid"]
    assert amax(out["de"][~valid[:, None, :].expand_as(out["de"])]) == 0.0
    assert amax(out["dK"][~valid.t()[..., None].expand_as(out["dK"])]) == 0.0    # padded keys: exactly 0
    s = {}
    if "temp" in sens:            # the temperature x (1 + 1e-3)
        w = R.attention_fwd(d["Q"], d["K"], d["v"], d["lens"], d["prior"], temp * (1 + 1e-3), bounds=False)
        s["attn@temp*1.001"] = ratio(out["attn"], w["attn"], R.bound_attn(ref))
    if "key" in sens:             # the last valid key of utterance 0 dropped
        l2 = d["lens"].clone()
        l2[0] -= 1
        w = R.attention_fwd(d["Q"], d["K"], d["v"], l2, d["prior"], temp, bounds=False)
        s["logprob@key-1"] = ratio(out["logprob"][0], w["logprob"][0], R.bound_logprob(ref)[0])
    if "vchunk" in sens:          # one a-chunk of v zeroed
        v2 = d["v"].clone()
        v2[:64] = 0
        w = R.attention_grads(d["Q"], d["K"], v2, d["lens"], out["de"], bounds=False)
        s["dQ@v[:64]=0"] = ratio(out["dQ"], w["dQ"], gr["dQ_err"])
    if "shift" in sens:           # one query frame off: Q read one row later
        Q2 = torch.cat([d["Q"][1:], d["Q"][-1:]], 0)
        w = R.attention_grads(Q2, d["K"], d["v"], d["lens"], out["de"], bounds=False)
        s["dK@Q+1"] = ratio(out["dK"], w["dK"], gr["dK_err"])
        s["dv@Q+1"] = ratio(out["dv"], w["dv"], gr["dv_err"])
    if "detemp" in sens:          # the backward's 1/temp x (1 + 1e-3)
        w, _ = R.attention_de(out["attn"], out["p_save"], d["dattn"], d["dlp"], d["lens"], temp * (1 + 1e-3), prior=d["prior"] is not None)
        s["de@temp*1.001"] = ratio(out["de"], w, de_err)
    print("\n%-28s " % name + " ".join("%s %.3g" % kv for kv in r.items()) + ("  | sensitivity: " if s else "")
          + " ".join("%s %.3g" % kv for kv in s.items()))
    bad = {k: x for k, x in r.items() if not x <= 1.0}
    assert not bad, (name, bad)
    weak = {k: x for k, x in s.items() if not x >= SHARP}
    assert not weak, (name, weak)
    return out, ref, d


@pytest.mark.parametrize("A", [20, 64, 128, 192, 256, 320, 448, 576, 600, 640])
def test_attention_a_sizes(env, A):
    """1 / 2 / 3 / 4 waves per dQ/dK workgroup, idle waves (A 320, 448: 5 and 7 chunks), a partial last a-chunk (20, 600)"""
    nw, idle = dqdk_waves(A)
    c = make_attention(45, 2, 129, A, seed=A, prior=A % 128 != 0)
    check_attention(env, c, 0.9, "A=%d (waves %d%s)" % (A, nw, ", idle" if idle else ""), sens=("vchunk",) if A >= 128 else ())


@pytest.mark.parametrize("Lk", [1, 127, 128, 129, 257, 896])
def test_attention_key_counts(env, Lk):
    """one to seven 128-column score tiles up to the forward's LDS limit (L 896)"""
    c = make_attention(33, 2, Lk, 64, seed=Lk, prior=Lk % 2 == 1, lens=torch.tensor([Lk, max(1, Lk - 5)]))
    check_attention(env, c, 1.3, "L=%d" % Lk, sens=("temp",) if Lk == 129 else ())


@pytest.mark.parametrize("T", [1, 31, 33, 862])
def test_attention_query_counts(env, T):
    c = make_attention(T, 2, 40, 128, seed=T, prior=True)
    check_attention(env, c, 0.7, "T=%d" % T, sens=("shift", "detemp") if T > 1 else ())


def test_attention_lds_limits(env):
    """L 897 needs more forward LDS than there is: RuntimeError.  The backward still runs at 897 and raises at 1273."""
    L, ops = env
    c = make_attention(8, 1, 897, 64, seed=3, prior=False, lens=torch.tensor([897]))
    d = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in c.items()}
    with pytest.raises(RuntimeError):
        ops.AttentionScoresFn.apply(d["Q"], d["K"], d["v"], d["lens"], None, 1.0)
    ref = R.attention_fwd(d["Q"], d["K"], d["v"], d["lens"], None, 1.0, bounds=False)
    attn = ref["attn"].float().contiguous()
    dQ, dv = torch.empty_like(d["Q"]), torch.zeros(64, device="cuda")
    for Lk, ok in ((897, True), (1273, False)):
        Kx = torch.zeros(Lk, 1, 64, device="cuda")
        Kx[:897] = d["K"]
        ax = torch.zeros(1, 8, Lk, device="cuda")
        ax[..., :897] = attn
        dax = torch.zeros_like(ax)
        dax[..., :897] = d["dattn"]
        dex, dK = torch.empty_like(ax), torch.empty_like(Kx)
        dv.zero_()
        rc = L.lib().ft_attention_bwd(ptr(d["Q"]), ptr(Kx), ptr(d["v"]), ptr(d["lens"]), None, ptr(ax), None, ptr(dax), None, ptr(dex),
                                      ptr(dQ), ptr(dK), ptr(dv), 8, 1, Lk, 64, 1.0, L.stream())
        torch.cuda.synchronize()
        assert (rc == 0) == ok, (Lk, rc)
        if ok:
            de_ref, de_err = R.attention_de(ax, None, dax, None, d["lens"], 1.0, prior=False)
            gr = R.attention_grads(d["Q"], Kx, d["v"], d["lens"], dex)
            rs = [ratio(dex, de_ref, de_err), ratio(dQ, gr["dQ"], gr["dQ_err"]), ratio(dK, gr["dK"], gr["dK_err"]),
                  ratio(dv, gr["dv"], gr["dv_err"])]
            print("\nbwd L=897 de dQ dK dv", rs)
            assert max(rs) <= 1.0


def test_attention_data_chosen_paths(env):
    """Every data-chosen path of attention.hip in one batch, each proven from the inputs by the kernel's own rule:
      b 0: tile 0 (rows 0-31) bit-identical query rows (padded frames as the model makes them) with a prior that still differs per
           row -> uniform tile; tile 1 rows equal in columns 0-63 but not after -> the pre-filter's second pass; the partial last
           tile (rows 64-69) uniform too.
      b 1: one query row with |C2 q| just above 60 in a-chunk 1 only, just below 60 in a-chunk 2 -> forward sum form for that chunk
           of tile 0 only; backward sum form for the whole wave of a-chunk 1 (that row is one of its 32 rows).
      b 2: one key with |C2 k| > 60 in a-chunk 0 only -> backward sum form for that key alone; dattn = dlogprob = 0 on tile 1 ->
           zero-gradient early exit (dQ exactly 0 there).  NaN in K at l >= in_lens for b 1 and 2.
    Also: one row so peaked that fp32 p underflows (b 1, row 40)."""
    T, B, Lk, A = 70, 3, 257, 320
    c = make_attention(T, B, Lk, A, seed=11, prior=True, lens=torch.tensor([257, 200, 131]))
    Q, K = c["Q"], c["K"]
    Q[0:32, 0] = Q[0, 0]
    Q[32:64, 0] = Q[32, 0]
    Q[32:64, 0, 64:] = torch.randn(32, A - 64) * 0.7
    Q[64:70, 0] = Q[64, 0]
    hi, lo = 61.0 / R.C2, 59.0 / R.C2
    Q[5, 1, 64:128] = hi * torch.sign(torch.randn(64))
    Q[5, 1, 128:192] = lo * torch.sign(torch.randn(64))
    K[7, 2, 0:64] = hi * torch.sign(torch.randn(64))
    K[200:, 1] = float("nan")
    K[131:, 2] = float("nan")
    Q[40, 1] = K[3, 1] * 40.0                                    # tanh(q + k) ~ sign(k) on key 3 only: e there ~ sum |v| / temp
    c["v"] = c["v"].abs() * torch.sign(K[3, 1])
    c["dattn"][2, 32:64] = 0
    c["dlp"][2, 32:64] = 0
    # the paths, by the kernel's rule
    def tile_rows(b, t0):
        return Q[t0:min(t0 + 32, T), b]
    assert all(bool((tile_rows(0, t0) == tile_rows(0, t0)[0]).all()) for t0 in (0, 64))
    t1 = tile_rows(0, 32)
    assert bool((t1[:, :64] == t1[0, :64]).all()) and not bool((t1 == t1[0]).all())
    q1 = (C2F * Q[0:32, 1]).abs()
    assert bool((q1[:, 64:128] > R.EXP_SAFE).any()) and not bool((q1[:, 128:192] > R.EXP_SAFE).any()) and bool((q1[:, 128:192] > 0.9 * R.EXP_SAFE).any())
    keys = R.sum_form_keys(K, c["lens"])[:, 2]
    assert int(keys.sum()) == 1 and bool(keys[7])
    assert float(c["dattn"][2, 32:64].abs().max()) == 0 and float(c["dlp"][2, 32:64].abs().max()) == 0
    out, ref, d = check_attention(env, c, 0.85, "paths", sens=("temp", "key", "shift", "vchunk", "detemp"))
    assert float(out["dQ"][32:64, 2].abs().max()) == 0.0
    assert bool((ref["p"][1, 40] < 2.0 ** -149).any()), "the peaked row must underflow fp32"
    # the autograd entry gives the same forward values and dQ (plain stores) as the direct calls
    L, ops = env
    Qg, Kg, vg = (d[k].clone().requires_grad_(True) for k in ("Q", "K", "v"))
    at, lp = ops.AttentionScoresFn.apply(Qg, Kg, vg, d["lens"], d["prior"], 0.85)
    (at * d["dattn"] + lp * d["dlp"]).sum().backward()
    assert torch.equal(at, out["attn"]) and torch.equal(lp, out["logprob"]) and torch.equal(Qg.grad, out["dQ"])


def test_attention_bench_shape(env):
    """B 32, T 862, A 640, lengths and prior of bench.synth_batch / beta_binomial_prior_batch; reference in float64 on the device"""
    import bench
    bt = bench.synth_batch(32, 0)
    lens, outl = bt["in_lens"], bt["out_lens"]
    T, Lk = int(outl.max()), int(lens.max())
    c = make_attention(T, 32, Lk, 640, seed=862, prior=False, scale=0.5, vscale=0.05, lens=lens)
    c["prior"] = bench.beta_binomial_prior_batch(lens, outl, T, Lk)
    pad = torch.arange(T)[None, :, None] >= outl[:, None, None]
    pad_row = torch.randn(640, generator=torch.Generator().manual_seed(5)) * 0.5
    for b in range(32):                                          # padded frames: the projection of one zero LSTM output
        c["Q"][int(outl[b]):, b] = pad_row
    c["dattn"] = c["dattn"].masked_fill(pad, 0.0)
    c["dlp"] = c["dlp"].masked_fill(pad, 0.0)
    check_attention(env, c, 1.0, "bench B32 T862 A640", sens=("key", "vchunk"))


# ---------------------------------------------------------------------------------------------------------------- CTC
def ctc_inputs(B, T, Lk, seed, prior_like=True):
    """attention log-probabilities as the model makes them: log(p + 1e-20) + log(prior + 1e-20) (unnormalised, so alpha / beta
    run into the thousands over T 862), or plain log-softmax rows"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, Lk, generator=g) * 3
    if not prior_like:
        return torch.log_softmax(x, 2)
    p = torch.softmax(x, 2)
    pr = torch.rand(B, T, Lk, generator=g) ** 2
    return torch.log(p + 1e-20) + torch.log(pr + 1e-20)


def run_ctc_multi(L, lps, flags, in32, out32, blank, with_beta=1, gout=1.0):
    F_ = len(lps)
    B, T, Lk = lps[0].shape
    C = __import__("ctypes")
    work = torch.empty(L.lib().ft_attn_ctc_workspace_floats(F_ * B, T, Lk), device="cuda")
    loss = torch.empty(1, device="cuda")
    arr = (C.c_void_p * F_)(*[t.data_ptr() for t in lps])
    rev = (C.c_int32 * F_)(*flags)
    L.check(L.lib().ft_attn_ctc_fwd_multi(arr, rev, F_, ptr(in32), ptr(out32), float(blank), ptr(work), ptr(loss), B, T, Lk, with_beta,
                                          L.stream()), "ft_attn_ctc_fwd_multi")
    dl = [torch.full_like(t, float("nan")) for t in lps]
    darr = (C.c_void_p * F_)(*[t.data_ptr() for t in dl])
    gd = torch.tensor([gout], device="cuda")
    L.check(L.lib().ft_attn_ctc_bwd_multi(arr, rev, F_, ptr(in32), ptr(out32), float(blank), ptr(work), ptr(gd), darr, B, T, Lk,
                                          with_beta, L.stream()), "ft_attn_ctc_bwd_multi")
    torch.cuda.synchronize()
    return loss[0], dl


def check_ctc(env, lps, flags, in_lens, out_lens, blank, name, sens=(), with_beta=1, gout=0.37):
    L, ops = env
    d = [t.cuda().contiguous() for t in lps]
    in32, out32 = in_lens.int().cuda(), out_lens.int().cuda()
    loss, dl = run_ctc_multi(L, d, flags, in32, out32, blank, with_beta, gout)
    assert math.isfinite(float(loss)) and all(bool(torch.isfinite(t).all()) for t in dl), name
    ref = R.ctc_multi_ref([t.double().cpu() for t in lps], flags, in_lens, out_lens, blank, gout)
    r = dict(loss=ratio(loss.cpu() / gout, ref["loss"] / gout, torch.tensor(float(ref["loss_err"]))))
    r["grad"] = max(ratio(g.cpu(), gr, ge) for g, gr, ge in zip(dl, ref["grads"], ref["grad_errs"]))
    s = {}
    F_ = len(lps)

    def wrong(lps_, flags_, il, ol, bl):
        w = R.ctc_multi_ref([t.double().cpu() for t in lps_], flags_, il, ol, bl, gout, bounds=False)
        return max(ratio(g.cpu(), gw, ge) for g, gw, ge in zip(dl, w["grads"], ref["grad_errs"]))
    if "K-1" in sens:
        il = in_lens.clone()
        il[0] -= 1
        s["grad@K0-1"] = wrong(lps, flags, il, out_lens, blank)
    if "T-1" in sens:
        ol = out_lens.clone()
        ol[0] -= 1
        s["grad@T0-1"] = wrong(lps, flags, in_lens, ol, blank)
    if "blank" in sens:
        s["grad@blank-0.01"] = wrong(lps, flags, in_lens, out_lens, blank - 0.01)
    if "unmirrored" in sens:
        s["grad@unmirrored"] = wrong(lps, [0] * F_, in_lens, out_lens, blank)
    print("\n%-28s " % name + " ".join("%s %.3g" % kv for kv in r.items()) + ("  | sensitivity: " if s else "")
          + " ".join("%s %.3g" % kv for kv in s.items()))
    # zero gradient on padded rows / columns and on infeasible samples, exactly
    for f, g in enumerate(dl):
        gc = g.cpu()
        for b in range(gc.shape[0]):
            Tb, Kb = int(out_lens[b]), int(in_lens[b])
            assert amax(gc[b, Tb:]) == 0.0 and amax(gc[b, :, Kb:]) == 0.0
            if not bool(ref["feasible"][f * gc.shape[0] + b]):
                assert float(gc[b].abs().max()) == 0.0
    bad = {k: x for k, x in r.items() if not x <= 1.0}
    assert not bad, (name, bad)
    weak = {k: x for k, x in s.items() if not x >= SHARP}
    assert not weak, (name, weak)
    return loss, dl, ref


@pytest.mark.parametrize("blank", [-8.0, -1.0])
def test_ctc_bench_shape(env, blank):
    """B 32, 2 flows, flow 1 in reversed time, T 862, L from bench.synth_batch"""
    import bench
    bt = bench.synth_batch(32, 1)
    il, ol = bt["in_lens"], bt["out_lens"]
    T, Lk = int(ol.max()), int(il.max())
    lps = [ctc_inputs(32, T, Lk, 100 + f) for f in range(2)]
    loss, dl, ref = check_ctc(env, lps, [0, 1], il, ol, blank, "ctc bench blank %g" % blank, sens=("K-1", "T-1", "unmirrored"))
    assert float(ref["alpha"][torch.isfinite(ref["alpha"])].abs().max()) > 1000.0      # the magnitudes the bound is about


def test_ctc_short_lengths(env):
    """T_b 1..9 (every tail of the 4-step prefetch groups of alpha and beta), T_b = K_b (single path), T_b < K_b (zero loss and
    gradient), K_b = 1; NaN in the padding of lp (rows t >= T_b, columns k >= K_b) must never be read"""
    ol = torch.tensor([1, 2, 3, 4, 5, 6, 7, 8, 9, 5, 3, 7])
    il = torch.tensor([1, 1, 2, 3, 3, 4, 5, 8, 6, 5, 6, 1])
    lp = ctc_inputs(12, 9, 8, 7, prior_like=False)
    for b in range(12):
        lp[b, int(ol[b]):] = float("nan")
        lp[b, :, int(il[b]):] = float("nan")
    assert bool((ol == il).any()) and bool((ol < il).any()) and bool((il == 1).any())
    check_ctc(env, [lp], [0], il, ol, -8.0, "ctc T_b 1..9", sens=("K-1", "T-1", "blank"))


def test_ctc_max_states(env):
    """L 511: 1023 states, 1024-thread workgroups, T ~ 1100; L 512 is refused"""
    L, ops = env
    il, ol = torch.tensor([511, 300]), torch.tensor([1100, 900])
    lp = ctc_inputs(2, 1100, 511, 9)
    check_ctc(env, [lp], [1], il, ol, -8.0, "ctc L511 T1100", sens=("unmirrored",))
    lp2 = torch.zeros(1, 4, 512, device="cuda")
    with pytest.raises(RuntimeError):
        ops.AttnCTCFn.apply(lp2, torch.tensor([512], dtype=torch.int32, device="cuda"), torch.tensor([4], dtype=torch.int32, device="cuda"), -1.0)


def test_ctc_with_beta_is_bit_identical(env):
    """with_beta 0 runs ctc_beta_k in the backward, 1 runs the same ctc_beta_body inside the forward launch: identical gradients.
    The loss is a float atomic sum over samples in an unspecified order: equal to rounding only."""
    L, ops = env
    il, ol = torch.tensor([20, 13, 13, 4]), torch.tensor([90, 61, 33, 11])
    lps = [ctc_inputs(4, 90, 20, 40 + f).cuda() for f in range(2)]
    l1, d1 = run_ctc_multi(L, lps, [0, 1], il.int().cuda(), ol.int().cuda(), -8.0, with_beta=1)
    l0, d0 = run_ctc_multi(L, lps, [0, 1], il.int().cuda(), ol.int().cuda(), -8.0, with_beta=0)
    assert all(torch.equal(a, b) for a, b in zip(d0, d1))
    assert abs(float(l0) - float(l1)) <= 8 * R.U * abs(float(l1))


@pytest.mark.parametrize("flags", [[1], [0, 0], [1, 0, 0], [1, 0, 0, 1, 1, 0, 1, 0]])
def test_ctc_multi_flags(env, flags):
    """F 1, 2, 3, 8 with reversal flags other than 'odd flows'"""
    il, ol = torch.tensor([17, 9, 9, 3, 1]), torch.tensor([60, 41, 9, 25, 13])
    lps = [ctc_inputs(5, 60, 17, 60 + f) for f in range(len(flags))]
    check_ctc(env, lps, flags, il, ol, -8.0, "ctc F=%d %s" % (len(flags), "".join(map(str, flags))),
              sens=("unmirrored",) if any(flags) else ("T-1",))


def test_ctc_multi_rejects_nine_flows(env):
    L, ops = env
    lp = torch.zeros(1, 4, 3, device="cuda")
    C = __import__("ctypes")
    arr = (C.c_void_p * 9)(*([lp.data_ptr()] * 9))
    rev = (C.c_int32 * 9)(*([0] * 9))
    work = torch.empty(L.lib().ft_attn_ctc_workspace_floats(9, 4, 3), device="cuda")
    loss = torch.empty(1, device="cuda")
    one = torch.tensor([3], dtype=torch.int32, device="cuda")
    rc = L.lib().ft_attn_ctc_fwd_multi(arr, rev, 9, ptr(one), ptr(one), -1.0, ptr(work), ptr(loss), 1, 4, 3, 1, L.stream())
    assert rc != 0


def test_flowtron_loss_ctc_term(env):
    """the ops.FlowtronLossFn entry (odd flows reversed) gives the same CTC value and gradient bits as the direct multi call"""
    L, ops = env
    il, ol = torch.tensor([12, 7, 7]), torch.tensor([40, 29, 17])
    T, B, M = 40, 3, 4
    lps = [ctc_inputs(B, T, 12, 80 + f).cuda().requires_grad_(True) for f in range(2)]
    z = torch.randn(T, B, M, device="cuda")
    nll, gl, ctc = ops.FlowtronLossFn.apply(z, None, None, ol.int().cuda(), il.int().cuda(), 1.0, -8.0, 0, *lps)
    ctc.backward()
    loss, dl = run_ctc_multi(L, [t.detach() for t in lps], [0, 1], il.int().cuda(), ol.int().cuda(), -8.0)
    ref = R.ctc_multi_ref([t.detach().double().cpu() for t in lps], [0, 1], il, ol, -8.0)
    assert ratio(ctc.detach().cpu(), ref["loss"], torch.tensor(float(ref["loss_err"]))) <= 1.0
    assert all(torch.equal(t.grad, g) for t, g in zip(lps, dl))
