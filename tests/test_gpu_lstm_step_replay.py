"""(-m gpu) The LAUNCH-PER-STEP LSTM kernels (csrc/lstm.hip, csrc/lstm2.hip) replayed step by step in float64.

These kernels run whenever the persistent ones do not (a timed-out launch or a failed self-test, FLOWTRON_LSTM_PERSIST=0, the fp32
parity mode, a reverse layer, a hidden size that cannot be padded to 1024), and they are the yardstick the persistent kernels are
proved bit-identical to.  tests/lstm_replay.py holds the replay, its bounds and the derivation of the accumulation constants;
tests/test_lstm_replay_cpu.py proves bounds and mutations on an emulation.  Every case calls the C entry directly, pre-fills the
outputs with 7.0, sizes the workspace with the project's *_workspace_bytes, uses ragged lengths that contain T and 1, asserts pad
rows of y / dgx exactly 0 (the helpers do) and prints its [replay ...] line.

Which template instantiation a case executes is part of its id (a: fwd<MODE,MT,G>xTRIPS / bwd<MT,G>xTRIPS of lstm_fwd_step /
lstm_bwd_step_bf16; c: lstm_fwd_pair / lstm_bwd_pair; d: the lstm2 kernel names).

Observed on the MI355X (worst ratio per kernel family over all cases of the family; replay must be <= 1, mutations >= 10), with the
derived accumulation constants c_acc (lstm_replay.c_acc_of):

  family (kernels)                                   c_acc (H = 1024)         replay   w       row      step
  seq16 fwd   lstm_fwd_step<1,..>                    H/128 + 4    (12)        0.50     111     1.1e6    8.2e5
  seq16 bwd   lstm_bwd_step_bf16                     H/128 + 16   (24)        0.20     75      8.9e5    5.2e6
  seq32 fwd   lstm_fwd_step<0,..>                    16 ceil(ceil(H/16)/4)+4  0.48     340     3.0e6    9.4e5     (w: rounded to bf16)
  seq32 bwd   lstm_bwd_pointwise + lstm_bwd_matmul   16 ceil(ceil(H/16)/4)+7  0.12     298     1.3e7    1.3e6     (w: rounded to bf16)
  bidir fwd   lstm_fwd_pair                          H/128 + 4    (12)        0.50     101     1.0e6    9.4e5
  bidir bwd   lstm_bwd_pair                          H/128 + 16   (24)        0.20     61      3.6e7    6.6e6
  lstm2 fwd   layer 0                                H/128 + 4    (12)        0.49     101     9.6e5    8.2e5
  lstm2 fwd   layer 1 (gx_tol: 2 H/128 + 4 = 20)     H/128 + 4    (12)        0.49     33      2.5e5    1.9e5
  lstm2 bwd   layer 1                                H/128 + 16   (24)        0.17     79      3.0e7    1.5e7
  lstm2 bwd   layer 0 (dy_tol: 2 H/128 + 16 = 32;    H/128 + 16   (24)        0.14     28      2.2e5    1.8e5
              lstm2_bwd_skew2: 40)
  lstm2, FT_LSTM2_BOTH=0 FT_LSTM2_SKEW2=0 (fwd l0 / l1 / bwd l1 / l0, the constants above, dy_tol 32)
                                                                              0.49     43      2.9e5    1.9e5
  weight gradients (gemm_ref64's bound)                                       0.15     a reference shifted the wrong way: 4.0e5

The replay figure of the forward families is the cell update's (2 u, nearly attained); the gates stay below 0.3 of their bound.
Before tests/lstm_replay.make_weight the fp16 `w` mutation of the two-layer chain scored 4 .. 9 on dense weights (its docstring).
Every instantiation the launchers can reach has a case (the ids name them); lstm_fwd_step<1,4,8,*> and lstm2_fwd_step<*,*,8> are
compiled but no shape reaches them (G = 8 is taken only at MT <= 2; the 8-wave forward is switched off in ft_lstm2_seq_fwd).
"""
import os
import subprocess
import sys

import pytest
import torch

import gemm_ref64 as G
import lstm_replay as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}                                      # family -> [worst replay ratio, {mutation: smallest ratio}]


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.lib()
    return L, ops


def print_table():
    for fam in sorted(WORST):
        print("[replay table] %-20s replay %.3f  mutations %s" % (fam, WORST[fam][0], {k: round(v, 1) for k, v in WORST[fam][1].items()}))


@pytest.fixture(autouse=True)
def _keep_capsys(capsys):
    yield from R.keep_capsys(capsys)


def note(family, res):
    r, muts = res
    w = WORST.setdefault(family, [0.0, {}])
    w[0] = max(w[0], r)
    for k, v in muts.items():
        w[1][k] = min(w[1].get(k, float("inf")), v)


def group_of(n):
    return 8 if n % 8 == 0 else 4 if n % 4 == 0 else 2 if n % 2 == 0 else 1


def mt_of(B):
    return 1 if B <= 16 else 2 if B <= 32 else 4


def seq_inst(H, B):
    """the instantiations launch_fwd / launch_bwd_fused (csrc/lstm.hip) pick, and the trips of skinny_bf16's group loop"""
    per, mt = H // 128, mt_of(B)
    g = group_of(per)
    gf = 8 if (g == 8 and mt <= 2) else 4 if g >= 4 else g
    return "fwd<1,%d,%d>x%d-bwd<1,%d>x%d" % (mt, gf, per // gf, g, per // g)


def T_of(H, B):
    return 7 + (H // 128 + B) % 6


def work_bytes(n):
    return torch.empty(n, device="cuda", dtype=torch.uint8)


def seq_fwd(L, mode, gx, w, lens, reverse):
    T, B, H4 = gx.shape
    H = H4 // 4
    y, g, c = R.bufs(T, B, H, "cuda")
    work = work_bytes(L.lib().ft_lstm_workspace_bytes(B, H))
    fn = L.lib().ft_lstm_seq_fwd if mode == 0 else L.op16("ft_lstm_seq_fwd", mode)
    L.check(fn(L.ptr(gx), L.ptr(w), L.ptr(lens), L.ptr(y), H, L.ptr(g), L.ptr(c), L.ptr(work), T, B, H, int(reverse), mode, L.stream()),
            "ft_lstm_seq_fwd")
    torch.cuda.synchronize()
    return y, g, c


def seq_bwd(L, mode, dy, w, lens, g, c, reverse):
    T, B, H = c.shape
    dgx = torch.full((T, B, 4 * H), 7.0, device="cuda")
    work = work_bytes(L.lib().ft_lstm_workspace_bytes(B, H))
    fn = L.lib().ft_lstm_seq_bwd if mode == 0 else L.op16("ft_lstm_seq_bwd", mode)
    L.check(fn(L.ptr(dy), H, L.ptr(w), L.ptr(lens), L.ptr(g), L.ptr(c), L.ptr(dgx), L.ptr(work), T, B, H, int(reverse), mode, L.stream()),
            "ft_lstm_seq_bwd")
    torch.cuda.synchronize()
    return dgx


def seq_case(L, mode, H, B, T, reverse, seed, full=False, tag=""):
    gx, w, lens, dy = R.make_inputs(T, B, H, seed, full, "cuda")
    kf, kb = ("fwd32", "bwd32") if mode == 0 else ("fwd16", "bwd16")
    fam = "seq32" if mode == 0 else "seq16"
    name = "%s H %d B %d T %d mode %d rev %d %s" % (fam, H, B, T, mode, reverse, tag)
    y, g, c = seq_fwd(L, mode, gx, w, lens, reverse)
    note(fam + " fwd", R.check_fwd(name, gx, w, lens, y, g, c, mode, reverse, c_acc=R.c_acc_of(kf, H)))
    dgx = seq_bwd(L, mode, dy, w, lens, g, c, reverse)
    note(fam + " bwd", R.check_bwd(name, dy, w, lens, g, c, dgx, mode, reverse, c_acc=R.c_acc_of(kb, H)))


# ---- a. ft_lstm_seq_fwd / _bwd, 16-bit operands ---------------------------------------------------------------------------------------
SEQ16 = [(128, 1), (256, 17), (384, 32), (512, 33), (640, 5), (768, 64), (1024, 32), (1024, 64)]
SEQ16 += [(256, 3), (512, 9), (1024, 7), (512, 20), (128, 40)]          # the (MT, G) of lstm_fwd_step the shapes above leave out


@pytest.mark.parametrize("reverse", [False, True], ids=["fwdtime", "reverse"])
@pytest.mark.parametrize("fmt", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,B", SEQ16, ids=["H%d-B%d-%s" % (H, B, seq_inst(H, B)) for H, B in SEQ16])
def test_seq16_replays_step_by_step(env, H, B, fmt, reverse):
    """lstm_fwd_step<1, MT, G, REV> / lstm_bwd_step_bf16<1, G, REV> on every (MT, G) the launchers pick, with 1, 2, 3 and 5 trips of
    skinny_bf16's group loop (H 384 / 640 / 768, H 1024 at MT 4)"""
    L, ops = env
    seq_case(L, fmt, H, B, T_of(H, B), reverse, 1000 * fmt + H + B + int(reverse))


@pytest.mark.parametrize("fmt,reverse", [(1, False), (2, True)])
def test_seq16_single_step_and_full_length_rows(env, fmt, reverse):
    """T = 1 (one launch, no recurrent term) and a batch without pad rows"""
    L, ops = env
    seq_case(L, fmt, 384, 17, 1, reverse, 5 + fmt, tag="T1")
    seq_case(L, fmt, 640, 33, 8, reverse, 7 + fmt, full=True, tag="full")


# ---- b. fp32 parity -------------------------------------------------------------------------------------------------------------------
SEQ32 = [(16, 1), (16, 33), (20, 17), (20, 64), (36, 33), (68, 17), (68, 64), (256, 1), (256, 33)]


@pytest.mark.parametrize("reverse", [False, True], ids=["fwdtime", "reverse"])
@pytest.mark.parametrize("H,B", SEQ32, ids=["H%d-B%d-fwd<0,%d,1>-mm<%d>" % (H, B, mt_of(B), mt_of(B)) for H, B in SEQ32])
def test_seq32_parity_mode_replays_step_by_step(env, H, B, reverse):
    """mode 0: lstm_fwd_step<0, MT, 1, REV>, lstm_bwd_pointwise + lstm_bwd_matmul<MT>; H % 16 != 0 runs the k < K guard of skinny_f32 and
    the j < H guard of lstm_bwd_matmul (H 20, 36, 68, with B > 16 too); H 16 is one k-chunk: three of the four waves idle"""
    L, ops = env
    seq_case(L, 0, H, B, T_of(H, B), reverse, 3000 + H + B + int(reverse))


# ---- c. the bidirectional chain -------------------------------------------------------------------------------------------------------
BIDIR = [(128, 5), (384, 17), (1024, 32), (1024, 40)]
BIDIR += [(256, 5), (512, 5), (1024, 5), (256, 17), (512, 17), (128, 40), (256, 40)]    # the other (MT, G) of lstm_fwd_pair, lstm_bwd_pair<2>, <4>


def bidir_inst(H, B):
    per, mt = H // 128, mt_of(B)
    g = group_of(per)
    gf = 8 if (g == 8 and mt <= 2) else 4 if g >= 4 else g
    return "pair<%d,%d>-bwdpair<%d>" % (mt, min(gf, 4) if mt == 4 else gf, g)


@pytest.mark.parametrize("fmt", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,B", BIDIR, ids=["H%d-B%d-%s" % (H, B, bidir_inst(H, B)) for H, B in BIDIR])
def test_bidir_chain_replays_each_direction_on_its_half(env, H, B, fmt):
    """ft_lstm_bidir_seq_fwd / _bwd (lstm_fwd_pair<MT, G>, lstm_bwd_pair<G>): y and dy have row stride 2H; each direction replays on its
    half, and each half equals, bit for bit, what the single-direction entry writes (same body, same order): neither overwrites the
    other"""
    L, ops = env
    T = T_of(H, B)
    gf, wf, lens, dyf = R.make_inputs(T, B, H, 4000 + H + B + fmt, device="cuda")
    gr, wr, _, dyr = R.make_inputs(T, B, H, 4500 + H + B + fmt, device="cuda")
    y = torch.full((T, B, 2 * H), 7.0, device="cuda")
    gs = [torch.full((T, B, 4 * H), 7.0, device="cuda") for _ in range(2)]
    cs = [torch.full((T, B, H), 7.0, device="cuda") for _ in range(2)]
    nb = L.lib().ft_lstm_workspace_bytes(B, H)
    work = [work_bytes(nb), work_bytes(nb)]
    L.check(L.op16("ft_lstm_bidir_seq_fwd", fmt)(L.ptr(gf), L.ptr(gr), L.ptr(wf), L.ptr(wr), L.ptr(lens), L.ptr(y), 2 * H, L.ptr(gs[0]), L.ptr(gs[1]),
                                                 L.ptr(cs[0]), L.ptr(cs[1]), L.ptr(work[0]), L.ptr(work[1]), T, B, H, L.stream()), "ft_lstm_bidir_seq_fwd")
    torch.cuda.synchronize()
    yf, yr = y[..., :H].contiguous(), y[..., H:].contiguous()
    name = "bidir H %d B %d T %d fmt %d " % (H, B, T, fmt)
    note("bidir fwd", R.check_fwd(name + "dir 0", gf, wf, lens, yf, gs[0], cs[0], fmt, c_acc=R.c_acc_of("fwd16", H)))
    note("bidir fwd", R.check_fwd(name + "dir 1", gr, wr, lens, yr, gs[1], cs[1], fmt, reverse=True, c_acc=R.c_acc_of("fwd16", H)))
    assert torch.equal(yf, seq_fwd(L, fmt, gf, wf, lens, False)[0]) and torch.equal(yr, seq_fwd(L, fmt, gr, wr, lens, True)[0])
    dy = torch.cat([dyf, dyr], -1).contiguous()
    d = [torch.full((T, B, 4 * H), 7.0, device="cuda") for _ in range(2)]
    L.check(L.op16("ft_lstm_bidir_seq_bwd", fmt)(L.ptr(dy), 2 * H, L.ptr(wf), L.ptr(wr), L.ptr(lens), L.ptr(gs[0]), L.ptr(gs[1]), L.ptr(cs[0]),
                                                 L.ptr(cs[1]), L.ptr(d[0]), L.ptr(d[1]), L.ptr(work[0]), L.ptr(work[1]), T, B, H, L.stream()),
            "ft_lstm_bidir_seq_bwd")
    torch.cuda.synchronize()
    note("bidir bwd", R.check_bwd(name + "dir 0", dyf, wf, lens, gs[0], cs[0], d[0], fmt, c_acc=R.c_acc_of("bwd16", H)))
    note("bidir bwd", R.check_bwd(name + "dir 1", dyr, wr, lens, gs[1], cs[1], d[1], fmt, reverse=True, c_acc=R.c_acc_of("bwd16", H)))


# ---- d. the two-layer chain -----------------------------------------------------------------------------------------------------------
def lstm2_inputs(T, B, H, seed):
    gx0, w_hh0, lens, dy1 = R.make_inputs(T, B, H, seed, device="cuda")
    g = torch.Generator().manual_seed(seed + 1)
    w_ih1, w_hh1 = [R.make_weight(H, g).cuda() for _ in range(2)]
    b1 = (torch.randn(4 * H, generator=g) * 0.1).cuda()
    return gx0, w_hh0, w_ih1, b1, w_hh1, lens, dy1


def lstm2_fwd(L, fmt, gx0, w_hh0, w_ih1, b1, w_hh1, lens):
    T, B, H4 = gx0.shape
    H = H4 // 4
    o0, o1 = R.bufs(T, B, H, "cuda"), R.bufs(T, B, H, "cuda")
    work = work_bytes(L.lib().ft_lstm2_workspace_bytes(B, H))
    L.check(L.op16("ft_lstm2_seq_fwd", fmt)(L.ptr(gx0), L.ptr(w_hh0), L.ptr(w_ih1), L.ptr(b1), L.ptr(w_hh1), L.ptr(lens), L.ptr(o0[0]), L.ptr(o0[1]),
                                            L.ptr(o0[2]), L.ptr(o1[0]), L.ptr(o1[1]), L.ptr(o1[2]), L.ptr(work), T, B, H, L.stream()), "ft_lstm2_seq_fwd")
    torch.cuda.synchronize()
    return o0, o1


def lstm2_bwd(L, fmt, dy1, w_hh0, w_ih1, w_hh1, lens, g0, c0, g1, c1):
    T, B, H = c0.shape
    dgx0, dgx1 = torch.full((T, B, 4 * H), 7.0, device="cuda"), torch.full((T, B, 4 * H), 7.0, device="cuda")
    work = work_bytes(L.lib().ft_lstm2_workspace_bytes(B, H))
    L.check(L.op16("ft_lstm2_seq_bwd", fmt)(L.ptr(dy1), L.ptr(w_hh0), L.ptr(w_ih1), L.ptr(w_hh1), L.ptr(lens), L.ptr(g0), L.ptr(c0), L.ptr(g1), L.ptr(c1),
                                            L.ptr(dgx0), L.ptr(dgx1), L.ptr(work), T, B, H, L.stream()), "ft_lstm2_seq_bwd")
    torch.cuda.synchronize()
    return dgx0, dgx1


def lstm2_case(L, fmt, H, B, T, knobs_off=False, fam="lstm2"):
    """both layers, forward and backward, every step of each on its own.  Layer 1's gx = b1 + op16(y0) . op16(W_ih1)^T and layer 0's dy =
    op16(dgx1) . op16(W_ih1) exist only inside the kernels' accumulators: the replay derives them in float64 and carries the bound of
    the shared accumulator (lstm_replay: l2f1_in; l2b0_in, or l2b0_sk where lstm2_bwd_skew2 hands the product over through memory)"""
    gx0, w_hh0, w_ih1, b1, w_hh1, lens, dy1 = lstm2_inputs(T, B, H, 6000 + H + B + 10 * T + fmt)
    (y0, g0, c0), (y1, g1, c1) = lstm2_fwd(L, fmt, gx0, w_hh0, w_ih1, b1, w_hh1, lens)
    name = "%s H %d B %d T %d fmt %d " % (fam, H, B, T, fmt)
    note(fam + " fwd l0", R.check_fwd(name + "layer 0", gx0, w_hh0, lens, y0, g0, c0, fmt, c_acc=R.c_acc_of("fwd16", H)))
    y16, W = R.op16(y0, fmt), R.op16(w_ih1, fmt)
    gx1 = b1.double() + y16 @ W.t()
    gx_tol = R.c_acc_of("l2f1_in", H) * R.U32 * (b1.double().abs() + y16.abs() @ W.abs().t())
    note(fam + " fwd l1", R.check_fwd(name + "layer 1", gx1, w_hh1, lens, y1, g1, c1, fmt, gx_tol=gx_tol, c_acc=R.c_acc_of("l2f1", H)))
    del gx1, gx_tol, y16
    dgx0, dgx1 = lstm2_bwd(L, fmt, dy1, w_hh0, w_ih1, w_hh1, lens, g0, c0, g1, c1)
    note(fam + " bwd l1", R.check_bwd(name + "layer 1", dy1, w_hh1, lens, g1, c1, dgx1, fmt, c_acc=R.c_acc_of("bwd16", H)))
    d16 = R.op16(dgx1, fmt)                                          # (pad rows: exactly 0, just asserted)
    skew = H == 1024 and not knobs_off
    dy_tol = R.c_acc_of("l2b0_sk" if skew else "l2b0_in", H) * R.U32 * (d16.abs() @ W.abs())
    note(fam + " bwd l0", R.check_bwd(name + "layer 0", d16 @ W, w_hh0, lens, g0, c0, dgx0, fmt, dy_tol=dy_tol, c_acc=R.c_acc_of("l2b0", H)))


# (H, B, the T values, the kernels the case runs)
LSTM2 = [(128, 3, (9,), "fwd_step<1,1,4>-dualw-bwd_step<1>-dualw"),
         (256, 20, (3,), "fwd_step<2,2,4>-dualw-bwd_step<2>-dualw"),
         (512, 16, (2,), "fwd_step<1,4,4>-dualw-bwd_step<4>-dualw"),
         (384, 33, (1, 2, 3, 9), "fwd_step<4,1,4>x3-bwd_step<1>x3-two_skinny"),
         (768, 32, (9,), "fwd_step<2,2,4>x3-bwd_step<2>x3-two_skinny"),
         (1024, 7, (9,), "fwd_both<1,8>-bwd_skew2<8>"),
         (1024, 32, (1, 2, 3, 9), "fwd_both<2,8>-bwd_skew2<8>"),
         (1024, 64, (9,), "fwd_step<4,4,4>x2-two_skinny-bwd_skew2<8>-4tiles"),
         # the (MT, G) of lstm2_fwd_step the shapes above leave out (the dualw branch at MT 4 among them)
         (256, 3, (9,), "fwd_step<1,2,4>-dualw-bwd_step<2>-dualw"),
         (128, 20, (9,), "fwd_step<2,1,4>-dualw-bwd_step<1>-dualw"),
         (512, 20, (9,), "fwd_step<2,4,4>-dualw-bwd_step<4>-dualw"),
         (256, 40, (9,), "fwd_step<4,2,4>-dualw-bwd_step<2>-dualw"),
         (768, 64, (9,), "fwd_step<4,2,4>x3-bwd_step<2>x3-two_skinny")]
LSTM2_CASES = [(H, B, T, what) for H, B, Ts, what in LSTM2 for T in Ts]


@pytest.mark.parametrize("fmt", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,B,T,what", LSTM2_CASES, ids=["H%d-B%d-T%d-%s" % c for c in LSTM2_CASES])
def test_lstm2_chain_replays_both_layers_step_by_step(env, H, B, T, what, fmt):
    """ft_lstm2_seq_fwd / _bwd: the dualw and the two-skinny_bf16 branches of lstm2_fwd_body / lstm2_bwd_body, lstm2_fwd_both,
    lstm2_bwd_skew2, and the ends of the skewed chains (T = 1, 2, 3: forward launches s = 0..T, skew-2 backward s = T-1..-2)"""
    L, ops = env
    lstm2_case(L, fmt, H, B, T)


# ---- e. the knob paths of lstm2 at H = 1024 -------------------------------------------------------------------------------------------
def test_lstm2_knob_paths_in_a_fresh_process():
    """FT_LSTM2_BOTH=0 / FT_LSTM2_SKEW2=0 (read once per process): lstm2_fwd_step<MT, 8, 4> and lstm2_bwd_step<8> at H = 1024 replay
    the same way (the child runs cases (1024, 32) and (1024, 7) of (d) and exits non-zero on a failure)"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--knob-child"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, FT_LSTM2_BOTH="0", FT_LSTM2_SKEW2="0"), cwd=ROOT)
    with R._cap():
        print("\n" + "\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("[replay ")))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("[replay fwd]") == 8 and r.stdout.count("[replay bwd]") == 8, r.stdout[-3000:]


def _knob_child():
    for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("FT_LSTM2_BOTH") == "0" and os.environ.get("FT_LSTM2_SKEW2") == "0"
    from flowtron_amd import _lib as L
    L.lib()
    for H, B in ((1024, 32), (1024, 7)):
        for fmt in (1, 2):
            lstm2_case(L, fmt, H, B, 9, knobs_off=True, fam="lstm2 knobs")
    print_table()


# ---- f. the weight gradients around the kernels ---------------------------------------------------------------------------------------
GRAD_SHAPES = [(128, 5, 6), (256, 33, 4)]


def grad_ref(da, hp, fmt, C0=None):
    """sum over the rows of op(da)^T op(hp) in float64 with gemm_ref64's bound; the GEMM may split its K = rows reduction into as many
    slices as it has 32-wide k-steps (an upper limit: the bound grows with the slices)"""
    K = da.shape[0] * da.shape[1]
    a = G.round_op(da.reshape(K, -1), fmt).double().t()
    b = G.round_op(hp.reshape(K, -1), fmt).double().t()
    slices = 1 if fmt == G.F32 else -(-K // 32)
    return G.reference(a, b, alpha=1.0, beta=1.0, C0=torch.zeros(a.shape[0], b.shape[0], dtype=torch.float64, device=da.device), fmt=fmt,
                       slices=slices, split=slices > 1)


def check_grad(name, got, da, hp, da_wrong, hp_wrong, fmt):
    ref, bound = grad_ref(da, hp, fmt)
    r = G.ratio(got, ref, bound)
    wrong, wbound = grad_ref(da_wrong, hp_wrong, fmt)
    m = G.ratio(got, wrong, wbound)
    with R._cap():
        print("\n[replay grad] %-44s %.3f of tol;  shifted the wrong way %.1f" % (name, r, m))
    w = WORST.setdefault("weight grads", [0.0, {}])
    w[0], w[1]["shift"] = max(w[0], r), min(w[1].get("shift", float("inf")), m)
    assert r <= 1.0, (name, r)
    assert m >= G.SHARP, (name, "a reference shifted the wrong way in time is not told apart", m)


@pytest.mark.parametrize("reverse", [False, True], ids=["fwdtime", "reverse"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("H,B,T", GRAD_SHAPES)
def test_lstm_seq_fn_weight_gradient(env, monkeypatch, H, B, T, mode, reverse):
    """LSTMSeqFn through autograd on the launch-per-step kernels: dW_hh = sum_t op(dgx[t])^T op(y[t -+ 1]) of the kernel's own dgx and y
    (mode 0, the fp32 gemm_raw branch: operands as they are)"""
    L, ops = env
    monkeypatch.setenv("FLOWTRON_LSTM_PERSIST", "0")
    gx, w, lens, dy = R.make_inputs(T, B, H, 7000 + H + mode + int(reverse), device="cuda")
    gx.requires_grad_(True)
    w.requires_grad_(True)
    y = ops.LSTMSeqFn.apply(gx, w, lens, reverse, mode, None, False)
    y.backward(dy)
    torch.cuda.synchronize()
    dgx, yd = gx.grad, y.detach()
    lo, hi = (dgx[1:], yd[:-1]), (dgx[:-1], yd[1:])
    right, wrong = (hi, lo) if reverse else (lo, hi)
    check_grad("LSTMSeqFn dW_hh H %d B %d T %d mode %d rev %d" % (H, B, T, mode, reverse), w.grad, *right, *wrong, mode)


@pytest.mark.parametrize("fmt", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,B,T", GRAD_SHAPES)
def test_bilstm_seq_fn_weight_gradients(env, monkeypatch, H, B, T, fmt):
    """BiLSTMSeqFn on the launch-per-step pair chain: both dW_hh from dgx and the halves of y (row stride 2H)"""
    L, ops = env
    monkeypatch.setenv("FLOWTRON_LSTM_PERSIST", "0")
    gf, wf, lens, dyf = R.make_inputs(T, B, H, 7100 + H + fmt, device="cuda")
    gr, wr, _, dyr = R.make_inputs(T, B, H, 7200 + H + fmt, device="cuda")
    for t in (gf, gr, wf, wr):
        t.requires_grad_(True)
    y = ops.BiLSTMSeqFn.apply(gf, gr, wf, wr, lens, fmt)
    y.backward(torch.cat([dyf, dyr], -1))
    torch.cuda.synchronize()
    yd = y.detach()
    name = "BiLSTMSeqFn H %d B %d T %d fmt %d " % (H, B, T, fmt)
    check_grad(name + "dW_hh fwd", wf.grad, gf.grad[1:], yd[:-1, :, :H], gf.grad[:-1], yd[1:, :, :H], fmt)
    check_grad(name + "dW_hh rev", wr.grad, gr.grad[:-1], yd[1:, :, H:], gr.grad[1:], yd[:-1, :, H:], fmt)


@pytest.mark.parametrize("fmt", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,B,T", GRAD_SHAPES)
def test_lstm2_seq_fn_weight_gradients(env, H, B, T, fmt):
    """LSTM2SeqFn: dW_hh0, dW_hh1, dW_ih1 and db1 from the kernels' own dgx0 / dgx1 (dgx1 never leaves the node: the C entry run again
    on the node's saved tensors gives it, and its dgx0 must equal the node's bit for bit)"""
    L, ops = env
    gx0, w_hh0, w_ih1, b_ih1, w_hh1, lens, dy1 = lstm2_inputs(T, B, H, 7300 + H + fmt)
    b_hh1 = torch.zeros_like(b_ih1)
    for t in (gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1):
        t.requires_grad_(True)
    y1 = ops.LSTM2SeqFn.apply(gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens, fmt)
    _, _, _, _, y0, g0, c0, _, g1, c1 = y1.grad_fn.saved_tensors
    y1.backward(dy1)
    torch.cuda.synchronize()
    dgx0, dgx1 = lstm2_bwd(L, fmt, dy1, w_hh0.detach(), w_ih1.detach(), w_hh1.detach(), lens, g0, c0, g1, c1)
    assert torch.equal(dgx0, gx0.grad)
    y1d = y1.detach()
    name = "LSTM2SeqFn H %d B %d T %d fmt %d " % (H, B, T, fmt)
    check_grad(name + "dW_hh0", w_hh0.grad, dgx0[1:], y0[:-1], dgx0[:-1], y0[1:], fmt)
    check_grad(name + "dW_hh1", w_hh1.grad, dgx1[1:], y1d[:-1], dgx1[:-1], y1d[1:], fmt)
    check_grad(name + "dW_ih1", w_ih1.grad, dgx1, y0, dgx1[1:], y0[:-1], fmt)
    # db1: the fp32 column sum of dgx1 in any order (rows - 1 additions)
    rows = T * B
    d = dgx1.double().reshape(rows, -1)
    e = float(((b_ih1.grad.double() - d.sum(0)).abs() / (G.U * rows * d.abs().sum(0) + 1e-38)).max())
    assert e <= 1.0, e
    assert torch.equal(b_ih1.grad, b_hh1.grad)


def test_worst_ratios_per_kernel_family():
    """last in the file: the worst replay ratio and the smallest mutation ratio per kernel family over the cases that ran (the table
    in the module docstring is a copy of this output)"""
    with R._cap():
        print()
        print_table()
    for fam, (r, muts) in WORST.items():
        assert r <= 1.0 and all(v >= R.SHARP for v in muts.values()), (fam, r, muts)


if __name__ == "__main__":
    if "--knob-child" in sys.argv:
        _knob_child()
