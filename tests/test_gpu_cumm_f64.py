"""(-m gpu) ft_cumm_attn_fwd / _bwd against the float64 replay of tests/cumm_ref64.py, one frame at a time, element by element.

Every frame is replayed from the kernel's OWN saved state (attn[:, i-1], cumm_all[i], kproj_all[i]) with the kernel's operand rounding,
and every output element must stay within its propagated bound (cumm_ref64's docstring has the rule); each case prints its worst
error / bound per output.  All outputs start as NaN, so a row the kernel leaves out shows.  Each case asserts what ran: fused or chain
by the library's own answer (ft_cumm_attn_fused), persistent or one launch per frame by the library's own condition (a status word
supplied, FT_CUMM_PERSIST not 0, B * ceil(L / 32) <= the device's CU count).  The C ABI is called directly through _lib.

The wrong references that prove the bounds sharp run without a GPU (tests/test_cumm_ref64_cpu.py), at shapes of this file."""
import math

import pytest
import torch

import cumm_ref64 as R

pytestmark = pytest.mark.gpu
NF, K1, K2 = 32, 5, 3


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.lib()
    return L


def ratio(got, ref, mask=None):
    """max |got - ref.v| / ref.e; where the bound is 0 the kernel must be exact (else inf); NaN (an element never written) is inf"""
    err, bound = (got.double() - ref.v).abs(), ref.err()
    if mask is not None:
        mask = mask.expand_as(err)
        err, bound = err[mask], bound[mask]
    if err.numel() == 0:
        return 0.0
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max())


def run_case(L_, monkeypatch, *, T, Lk, lens, fmt, persist=True, split=None, chunk=None, ups="all", cls="aligned", w1_scale=0.3,
             E=640, A=640, temp=0.9, expect_fused=None, expect_persist=None, seed=0):
    lib = L_.lib()
    for k, v in (("FT_CUMM_FUSED", None), ("FT_CUMM_PERSIST", None if persist else "0"), ("FT_CUMM_SPLIT", split),
                 ("FT_CUMM_CHUNK", None if chunk is None else str(chunk))):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    B = len(lens)
    d, up = R.make_inputs(T, Lk, lens, E=E, A=A, seed=seed, cls=cls, w1_scale=w1_scale, device="cuda")
    if ups == "last":
        up["dctx"][:-1] = 0
    if ups == "first":
        up["dctx"][1:] = 0
    f = {k: t.float().contiguous() for k, t in d.items()}
    g = {k: t.float().contiguous() for k, t in up.items()}
    dattn, dlp = (g["dattn"], g["dlp"]) if ups == "all" else (None, None)
    lens32 = torch.tensor(lens, dtype=torch.int32, device="cuda")
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    ctx, attn, logprob, cumm_all, kproj = nan(T, B, A), nan(B, T, Lk), nan(B, T, Lk), nan(T, B, Lk), nan(T, Lk * B, A)
    nbytes = max(lib.ft_cumm_attn_workspace_bytes(T, Lk, B, E, A, NF, K1, K2, fmt, bw) for bw in (0, 1)) + 512
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    base = (work.data_ptr() + 255) // 256 * 256
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = L_.ptr
    args = L_.CummAttnArgs(p(f["text"]), p(f["Q"]), p(f["V"]), p(f["wk"]), p(f["v"]), p(f["w1"]), p(f["b1"]), p(f["w2"]), p(f["b2"]),
                           p(lens32), p(ctx), p(attn), p(logprob), p(cumm_all), p(kproj), base, nbytes - (base - work.data_ptr()),
                           T, B, Lk, E, A, NF, K1, K2, float(temp), int(fmt), p(status))
    import ctypes as C
    fused = bool(lib.ft_cumm_attn_fused(C.byref(args)))
    n_cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    persistent = fused and persist and B * math.ceil(Lk / R.FWD_ROWS) <= n_cu
    if expect_fused is not None:
        assert fused == expect_fused, "fused path: the library answers %s" % fused
    if expect_persist is not None:
        assert persistent == expect_persist, (B * math.ceil(Lk / R.FWD_ROWS), n_cu)
    L_.check(lib.ft_cumm_attn_fwd(C.byref(args), L_.stream()), "ft_cumm_attn_fwd")
    torch.cuda.synchronize()
    assert int(status.item()) == 0, "the persistent forward gave up a hand-off wait"
    dQ, dV, dtext = nan(T, B, A), nan(Lk, B, A), nan(Lk, B, E)
    dwk, dv, dw1, db1, dw2, db2 = nan(A, E), nan(A), nan(NF, 2, K1), nan(NF), nan(E, NF, K2), nan(E)
    L_.check(lib.ft_cumm_attn_bwd(C.byref(args), p(g["dctx"]), p(dattn), p(dlp), p(dQ), p(dV), p(dtext), p(dwk), p(dv), p(dw1), p(db1),
                                  p(dw2), p(db2), L_.stream()), "ft_cumm_attn_bwd")
    torch.cuda.synchronize()

    rfmt = fmt if fused else 0
    assert fused or fmt == 0, "the 16-bit launch chain is not replayed here (tests/test_gpu_ops.py holds it)"
    P = R.Params(**d, in_lens=lens, temp=temp)
    st = R.State(attn, cumm_all, kproj, P)
    vl = P.valid.t()[:, :, None]
    worst = {}

    def note(name, x):
        worst[name] = max(worst.get(name, 0.0), x)

    for i in range(T):
        assert torch.equal(cumm_all[i].double(), R.cumm_exact(st, i)), "cumm_all[%d] is not the fp32 sum cumm_all[i-1] + attn[:, i-1]" % i
        fr = R.frame_fwd(P, st, i, rfmt)
        note("tanh" if fused else "keys", ratio(st.kproj[i], fr["saved"], vl if fused else None))
        note("attn", ratio(attn[:, i], fr["attn"], P.valid))
        assert float(attn[:, i][~P.valid].abs().sum()) == 0.0 and not torch.isnan(attn[:, i]).any(), "attn beyond in_len must be zero"
        note("logprob", ratio(logprob[:, i], fr["logprob"]))
    note("ctx", ratio(ctx, R.ctx_ref(P, st, rfmt)))
    bw = R.replay_bwd(P, st, up["dctx"], up["dattn"] if ups == "all" else None, up["dlp"] if ups == "all" else None, rfmt, chunk=chunk)
    got = dict(dQ=dQ, dV=dV, dtext=dtext, dw_key=dwk, dv=dv, dw1=dw1, db1=db1, dw2=dw2, db2=db2)
    for k in R.OUT_BWD:
        note(k, ratio(got[k], bw[k]))
    for name, t in (("dtext", dtext), ("dV", dV)):
        assert float(t[~vl.expand_as(t)].abs().sum()) == 0.0, "%s beyond in_len must be zero" % name
    tag = "fused %s" % ("persistent" if persistent else "per-frame") if fused else "chain"
    print("\n[cumm f64 %s fmt %d T %d L %d lens %s %s%s%s %s] error / bound: %s" % (
        tag, fmt, T, Lk, lens, cls, " split=" + split if split else "", " chunk=%d" % chunk if chunk else "", ups,
        " ".join("%s %.3g" % kv for kv in worst.items())))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad
    return worst


# lengths: 1, L, multiples of the backward's 26 own rows and of the forward's 32, and those +- 1 and +- 3 (the 3-row halo and the
# convolutions' zero padding straddle the valid end)
MAIN = (33, [33, 27, 1])


@pytest.mark.parametrize("persist", [True, False])
@pytest.mark.parametrize("fmt", [1, 2])
def test_fused_frames_persistent_and_per_frame(env, monkeypatch, fmt, persist):
    run_case(env, monkeypatch, T=2, Lk=MAIN[0], lens=MAIN[1], fmt=fmt, persist=persist, expect_fused=True, expect_persist=persist)


@pytest.mark.parametrize("persist", [True, False])
def test_fused_frames_unsplit_items(env, monkeypatch, persist):
    """FT_CUMM_SPLIT=0: one workgroup walks both column halves of a tile"""
    run_case(env, monkeypatch, T=2, Lk=64, lens=[64, 55, 35], fmt=1, persist=persist, split="0", expect_fused=True, expect_persist=persist)


@pytest.mark.parametrize("fmt", [1, 2])
def test_fused_frames_three_frames_and_split_forced_on(env, monkeypatch, fmt):
    """T = 3 (the bound of the carry has passed through two frames) with FT_CUMM_SPLIT=1"""
    run_case(env, monkeypatch, T=3, Lk=MAIN[0], lens=MAIN[1], fmt=fmt, split="1", expect_fused=True, expect_persist=True)


@pytest.mark.parametrize("Lk,lens", [(1, [1]), (2, [2, 1, 1]), (3, [3, 2, 1]), (26, [26, 25, 23]), (27, [27, 26, 1]), (32, [32, 31, 29]),
                                     (52, [52, 51, 49]), (64, [53, 33, 29]), (64, [64, 35, 61]), (255, [255, 237, 195]),
                                     (256, [256, 255, 253]), (257, [257, 256, 211])])
def test_fused_frames_lengths(env, monkeypatch, Lk, lens):
    """L below the halo, at the tile edges of both kernels, at the 256-thread trip edge of softmax_block (255 / 256 / 257: one and two
    trips), lengths whose halo straddles the valid end (26 k +- 1, +- 3; 32 k +- 1, +- 3)"""
    run_case(env, monkeypatch, T=2, Lk=Lk, lens=lens, fmt=1 + (Lk % 2), expect_fused=True, expect_persist=True)


def test_fused_frames_at_the_length_limit(env, monkeypatch):
    """L = 1024 = the limit of ftint_cummf_supported: four softmax trips, 32 forward and 40 backward tiles per utterance; 96 tiles: persistent"""
    run_case(env, monkeypatch, T=2, Lk=1024, lens=[1024, 1023, 835], fmt=1, expect_fused=True, expect_persist=True)


def test_fused_frames_more_tiles_than_cus(env, monkeypatch):
    """B 9 x 32 tiles = 288 > 256 CUs: the default forward is one launch per frame BY GEOMETRY (status word supplied, no environment)"""
    run_case(env, monkeypatch, T=2, Lk=1024, lens=[1024, 1021, 1001, 989, 3, 1, 781, 806, 833], fmt=2, expect_fused=True, expect_persist=False)


@pytest.mark.parametrize("fmt", [1, 2])
def test_fused_frames_chunked_weight_gradients(env, monkeypatch, fmt):
    """FT_CUMM_CHUNK=4 at T = 9: three chunks, the top one partial, beta accumulation of dW_key / dw2 / db2 (a small first convolution
    keeps the never-reset carry bound from growing over the nine frames)"""
    run_case(env, monkeypatch, T=9, Lk=MAIN[0], lens=MAIN[1], fmt=fmt, chunk=4, w1_scale=1e-3, expect_fused=True)


@pytest.mark.parametrize("ups", ["dctx", "last", "first"])
def test_fused_frames_upstream_gradients(env, monkeypatch, ups):
    """dattn / dlogprob NULL; dctx only at the last frame; only at frame 0"""
    run_case(env, monkeypatch, T=2, Lk=MAIN[0], lens=MAIN[1], fmt=1, ups=ups, expect_fused=True)


def test_fused_frames_signed_inputs(env, monkeypatch):
    """N(0, 1) weights of both signs: the forward's bound is as tight, the backward's is valid but wide (cumm_ref64.make_inputs)"""
    run_case(env, monkeypatch, T=2, Lk=MAIN[0], lens=MAIN[1], fmt=1, cls="signed", expect_fused=True)


@pytest.mark.parametrize("fmt", [1, 2])
def test_length_1025_is_routed_to_the_chain(env, monkeypatch, fmt):
    """beyond ftint_cummf_supported's L <= 1024 the library must answer `chain` for the 16-bit modes (the 16-bit chain's values stay
    under tests/test_gpu_ops.py; the fp32 chain runs this length below)"""
    import ctypes as C
    a = env.CummAttnArgs()
    a.T, a.B, a.L, a.E, a.A, a.NF, a.K1, a.K2, a.mode, a.temperature = 2, 1, 1025, 640, 640, NF, K1, K2, fmt, 1.0
    assert env.lib().ft_cumm_attn_fused(C.byref(a)) == 0
    a.L = 1024
    assert env.lib().ft_cumm_attn_fused(C.byref(a)) == 1


@pytest.mark.parametrize("E,A,T,Lk,lens,cls", [(40, 48, 3, 33, [33, 27, 1], "aligned"), (40, 48, 3, 33, [33, 27, 1], "signed"),
                                               (640, 640, 2, 33, [33, 27, 1], "aligned"), (640, 640, 2, 33, [33, 27, 1], "signed"),
                                               (640, 640, 2, 1025, [1025], "aligned")])
def test_fp32_launch_chain(env, monkeypatch, E, A, T, Lk, lens, cls):
    """csrc/cumm_attn.hip in fp32 mode, at a small width, at 640 and at the length the fused path refuses: pure fp32 bounds, no 16-bit
    rounding and no ambiguity term"""
    run_case(env, monkeypatch, T=T, Lk=Lk, lens=lens, fmt=0, E=E, A=A, cls=cls, expect_fused=False)


def test_matrix_instruction_with_a_subnormal_fp16_operand(env):
    """the measurement behind cumm_ref64.lifted: two exact products with a subnormal fp16 operand, summed inside one matrix instruction
    (ft_gemm, fp16 mode), need not give the exact fp32 sum -- the deviation must stay within the bound that weighs the subnormal as
    the smallest normal; with both operands scaled by 1024 (normal) and in bf16 (operands rounded) the bound without lifting holds"""
    from flowtron_amd import ops
    q = 2.0 ** -24
    w0, w1 = 1.41210938, 0.0148849487                                  # 1446 x 2^-10 and 1951 x 2^-17: fp16 numbers
    for scale in (1.0, 1024.0):
        x, W = torch.zeros(1, 1, 32, device="cuda"), torch.zeros(16, 32, device="cuda")
        x[0, 0, 0], x[0, 0, 1] = q * scale, -q * scale
        W[0, 0], W[0, 1], W[1, 0], W[2, 1] = w0, w1, w0, w1
        y = ops.linear([x], W, None, act=0, mode=2).double().flatten()
        a, w = x.double().reshape(1, 32), W.double()
        ref = R.lin(lambda a_, w_: a_ @ w_.t(), R.EV(a), w, R.n_lib(32, 2), 32, 2)
        r = ratio(y[:3], R.EV(ref.v.flatten()[:3], ref.e.flatten()[:3]))
        print("\n[fp16 operand %g x 2^-24] sum, products in units of 2^-41: %s (exact 183137, 185088, -1951); error / bound %.3g" % (
            scale, (y[:3] / scale / 2.0 ** -41).tolist(), r))
        assert r <= 1.0
        assert float(y[1]) == float(a[0, 0] * w[1, 0]) and float(y[2]) == float(a[0, 1] * w[2, 1]), "a single product must be exact"
        if scale > 1:
            assert float(y[0]) == float(ref.v[0, 0]), "normal operands: the two-term sum is exact"
