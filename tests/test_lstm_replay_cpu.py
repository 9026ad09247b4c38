"""tests/lstm_replay.py checked on the CPU against a plain torch emulation of one recurrence kernel: operands rounded to the operand
format, fp32 accumulation in a shuffled chunk order dealt to several partial sums (one rounding per 32-wide chunk for the 16-bit
formats, one fused rounding per k for fmt 0 -- the helper's model of the matrix instructions), fp32 cell math.  The emulation must
replay with every ratio <= 1 under the constant that its own accumulation derives (chunks per partial sum + the additions of the
partial sums), and every mutation (`w`, `row`, `step`; fmt 0: the inverted `w`) must score >= SHARP.  The two-layer chain of
csrc/lstm2.hip is emulated the same way: the layer-1 gx_tol and the layer-0 backward dy_tol are exercised with both K segments in
one accumulator.

This is also where the input scales of tests/test_gpu_lstm_step_replay.py are chosen (lstm_replay.make_inputs): gx ~ 0.5 N(0, 1), dy ~ 0.1 N(0, 1), and
weights with sparse, large rows and columns among the dense ones (lstm_replay.make_weight says why)."""
import pytest
import torch

import lstm_replay as R

F32 = torch.float32


@pytest.fixture(autouse=True)
def _keep_capsys(capsys):
    yield from R.keep_capsys(capsys)


inputs = R.make_inputs


def chain(a, w, fmt, nparts, gen):
    """partial sums (fp32) of a [B, K] . w [N, K]^T, a and w float64 holding operand-format values: the chunks in a shuffled order dealt
    to `nparts` accumulators, ONE fp32 rounding per chunk (products and the sum inside a chunk exact in float64).  Returns (parts,
    chunks on the longest accumulator)."""
    K = a.shape[1]
    width = 1 if fmt == 0 else 32
    chunks = [(k, min(k + width, K)) for k in range(0, K, width)]
    perm = torch.randperm(len(chunks), generator=gen).tolist()
    parts = []
    for p in range(nparts):
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=F32)
        for i in perm[p::nparts]:
            k0, k1 = chunks[i]
            acc = (acc.double() + a[:, k0:k1] @ w[:, k0:k1].t()).to(F32)
        parts.append(acc)
    return parts, -(-len(chunks) // nparts)


def emu_c_acc(K, fmt, nparts):
    return -(-(-(-K // (1 if fmt == 0 else 32))) // nparts) + nparts


def rows_at(x, t_b):
    return x[t_b, torch.arange(t_b.numel())]


def emu_fwd(gx, w, lens, fmt, reverse=False, nparts=4, seed=0, x_seq=None, w_in=None):
    """one forward recurrence as the step kernels run it; x_seq / w_in: layer 1 of the two-layer chain -- gx is then the bias [4H] and
    the input product x_seq[t] . w_in^T shares the accumulators with the recurrent one"""
    gen = torch.Generator().manual_seed(seed)
    T, B = (x_seq.shape[0], x_seq.shape[1]) if x_seq is not None else gx.shape[:2]
    Hd = w.shape[1]
    W = R.op16(w, fmt) if x_seq is None else torch.cat([R.op16(w_in, fmt), R.op16(w, fmt)], 1)
    y = torch.zeros(T, B, Hd)
    gates, cell = torch.full((T, B, 4 * Hd), 7.0), torch.full((T, B, Hd), 7.0)
    h, c = torch.zeros(B, Hd), torch.zeros(B, Hd)
    b = torch.arange(B)
    ln = lens.long()
    for s in range(T):
        act = s < ln
        t_b = torch.where(act, (ln - 1 - s) if reverse else torch.full_like(ln, s), torch.zeros_like(ln))
        a = R.op16(h, fmt) if x_seq is None else torch.cat([R.op16(rows_at(x_seq, t_b), fmt), R.op16(h, fmt)], 1)
        parts, _ = chain(a, W, fmt, nparts, gen)
        pre = rows_at(gx, t_b) if x_seq is None else gx[None, :].expand(B, -1).clone()
        for p in parts:
            pre = pre + p
        zi, zf, zg, zo = pre.chunk(4, -1)
        ig, fg, gg, og = torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)
        c_new = (fg.double() * c.double() + (ig * gg).double()).to(F32)               # fma(f, c, i * g)
        h_new = og * torch.tanh(c_new)
        rows = b[act]
        y[t_b[act], rows] = h_new[act]
        gates[t_b[act], rows] = torch.cat([ig, fg, gg, og], -1)[act]
        cell[t_b[act], rows] = c_new[act]
        h, c = torch.where(act[:, None], h_new, h), torch.where(act[:, None], c_new, c)
    return y, gates, cell


def emu_bwd(dy, w, lens, g, c, fmt, reverse=False, nparts=16, seed=0, d_in=None, w_in=None):
    """one backward recurrence; d_in / w_in: layer 0 of the two-layer chain -- no external dy, dh = dgates1[t] . W_ih1 + dgates0_next .
    W_hh0 in shared accumulators"""
    gen = torch.Generator().manual_seed(seed)
    T, B, Hd = c.shape
    Wt = R.op16(w, fmt).t() if d_in is None else torch.cat([R.op16(w_in, fmt), R.op16(w, fmt)], 0).t()      # [H, 4H (8H)]
    dgx = torch.full((T, B, 4 * Hd), 7.0)
    da_prev, carry = torch.zeros(B, 4 * Hd), torch.zeros(B, Hd)
    b = torch.arange(B)
    ln = lens.long()
    for s in reversed(range(T)):
        act = s < ln
        t_b = torch.where(act, (ln - 1 - s) if reverse else torch.full_like(ln, s), torch.full_like(ln, s))
        a = R.op16(da_prev, fmt) if d_in is None else torch.cat([R.op16(rows_at(d_in, t_b), fmt), R.op16(da_prev, fmt)], 1)   # (pad rows of d_in: 0)
        parts, _ = chain(a, Wt, fmt, nparts, gen)
        dh = rows_at(dy, t_b).clone() if d_in is None else torch.zeros(B, Hd)
        for p in parts:
            dh = dh + p
        gt = torch.where(act[:, None], rows_at(g, t_b), torch.zeros(()))
        ig, fg, gg, og = gt.chunk(4, -1)
        c_t = torch.where(act[:, None], rows_at(c, t_b), torch.zeros(()))
        tp = (t_b + 1 if reverse else t_b - 1).clamp(0, T - 1)
        c_prev = torch.where(act[:, None], rows_at(c, tp), torch.zeros(())) if s > 0 else torch.zeros(B, Hd)
        tc = torch.tanh(c_t)
        om = (1.0 - tc.double() * tc.double()).to(F32)                                  # fma(-tc, tc, 1)
        dc = ((dh * og).double() * om.double() + carry.double()).to(F32)                # fma(dh o, 1 - tc^2, carry)
        da = torch.cat([dc * gg * ig * (1 - ig), dc * c_prev * fg * (1 - fg), dc * ig * (1 - gg * gg), dh * tc * og * (1 - og)], -1)
        da = torch.where(act[:, None], da, torch.zeros(()))
        dgx[t_b, b] = da
        carry = torch.where(act[:, None], dc * fg, carry)
        da_prev = da
    return dgx


SHAPES = {0: [(20, 3, 7, 4), (36, 17, 8, 4), (16, 1, 9, 4)], 1: [(64, 5, 9, 2), (96, 17, 7, 3)], 2: [(64, 5, 9, 2), (96, 17, 7, 3)]}
CASES = [(fmt, Hd, B, T, nparts) for fmt in (0, 1, 2) for (Hd, B, T, nparts) in SHAPES[fmt]]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("fmt,Hd,B,T,nparts", CASES)
def test_emulated_recurrence_replays_and_mutations_are_caught(fmt, Hd, B, T, nparts, reverse):
    gx, w, lens, dy = inputs(T, B, Hd, 100 * fmt + Hd + B)
    y, g, c = emu_fwd(gx, w, lens, fmt, reverse, nparts, seed=Hd)
    name = "emulation fmt %d H %d B %d T %d rev %d" % (fmt, Hd, B, T, reverse)
    r, muts = R.check_fwd(name, gx, w, lens, y, g, c, fmt, reverse, c_acc=emu_c_acc(Hd, fmt, nparts))
    assert set(muts) == set(R.sharp_muts(lens, B))
    dgx = emu_bwd(dy, w, lens, g, c, fmt, reverse, 4 * nparts, seed=Hd + 1)
    R.check_bwd(name, dy, w, lens, g, c, dgx, fmt, reverse, c_acc=emu_c_acc(4 * Hd, fmt, 4 * nparts))


def test_single_step_and_full_length_rows():
    """T = 1: nothing recurrent to mutate, the replay still holds; every row full length: no pad row at all"""
    gx, w, lens, dy = inputs(1, 5, 64, 3)
    y, g, c = emu_fwd(gx, w, lens, 1)
    assert R.sharp_muts(lens, 5) == []
    R.check_fwd("emulation T 1", gx, w, lens, y, g, c, 1, c_acc=emu_c_acc(64, 1, 4))
    R.check_bwd("emulation T 1", dy, w, lens, g, c, emu_bwd(dy, w, lens, g, c, 1), 1, c_acc=emu_c_acc(256, 1, 16))
    gx, w, lens, dy = inputs(6, 4, 64, 4, full=True)
    y, g, c = emu_fwd(gx, w, lens, 2, reverse=True)
    R.check_fwd("emulation full rows", gx, w, lens, y, g, c, 2, True, c_acc=emu_c_acc(64, 2, 4))
    R.check_bwd("emulation full rows", dy, w, lens, g, c, emu_bwd(dy, w, lens, g, c, 2, True), 2, True, c_acc=emu_c_acc(256, 2, 16))


def test_a_wrong_kernel_is_caught():
    """the replay itself fails on an emulation that is subtly wrong: a dropped k-chunk, the bias / gx added twice, a wrong batch row"""
    gx, w, lens, dy = inputs(8, 6, 64, 11)
    ca = emu_c_acc(64, 1, 4)
    w_drop = w.clone()
    w_drop[:, 32:64] = 0                                             # the kernel skips the second k-chunk
    y, g, c = emu_fwd(gx, w_drop, lens, 1)
    assert R.replay_fwd(gx, w, lens, y, g, c, 1, c_acc=ca)[0] >= R.SHARP
    y, g, c = emu_fwd(2 * gx, w, lens, 1)
    assert R.replay_fwd(gx, w, lens, y, g, c, 1, c_acc=ca)[0] >= R.SHARP
    y, g, c = emu_fwd(gx, w, lens, 1)
    y2 = y.clone()
    assert int(lens[2]) == 8 and int(lens[5]) == 8
    y2[2, 2], y2[2, 5] = y[2, 5], y[2, 2]                            # two rows of a tile swapped in one step
    assert max(R.replay_fwd(gx, w, lens, y2, g, c, 1, c_acc=ca)) >= R.SHARP
    dgx = emu_bwd(dy, w_drop, lens, g, c, 1)
    assert R.replay_bwd(dy, w, lens, g, c, dgx, 1, c_acc=emu_c_acc(256, 1, 16)) >= R.SHARP


@pytest.mark.parametrize("fmt,Hd,B,T", [(1, 64, 5, 9), (2, 96, 17, 3), (1, 64, 3, 1), (2, 64, 4, 2)])
def test_emulated_two_layer_chain(fmt, Hd, B, T):
    """csrc/lstm2.hip's data flow: layer 1's gx is never materialised (bias + input product + recurrent product in one accumulator), nor
    is layer 0's dy in the backward: the replay derives them in float64 and carries their bounds as gx_tol / dy_tol"""
    gx0, w_hh0, lens, dy1 = inputs(T, B, Hd, 7 * Hd + B + fmt)
    g = torch.Generator().manual_seed(Hd + T)
    w_ih1, w_hh1 = [R.make_weight(Hd, g) for _ in range(2)]
    b1 = torch.randn(4 * Hd, generator=g) * 0.1
    y0, g0, c0 = emu_fwd(gx0, w_hh0, lens, fmt, seed=1)
    y1, g1, c1 = emu_fwd(b1, w_hh1, lens, fmt, seed=2, x_seq=y0, w_in=w_ih1)
    name = "emulated pair fmt %d H %d B %d T %d" % (fmt, Hd, B, T)
    R.check_fwd(name + " layer 0", gx0, w_hh0, lens, y0, g0, c0, fmt, c_acc=emu_c_acc(Hd, fmt, 4))
    ca = emu_c_acc(2 * Hd, fmt, 4)
    y16, W = R.op16(y0, fmt), R.op16(w_ih1, fmt)
    gx1 = b1.double() + y16 @ W.t()
    R.check_fwd(name + " layer 1", gx1, w_hh1, lens, y1, g1, c1, fmt, gx_tol=ca * R.U32 * (b1.double().abs() + y16.abs() @ W.abs().t()), c_acc=ca)
    dgx1 = emu_bwd(dy1, w_hh1, lens, g1, c1, fmt, seed=3)
    R.check_bwd(name + " layer 1", dy1, w_hh1, lens, g1, c1, dgx1, fmt, c_acc=emu_c_acc(4 * Hd, fmt, 16))
    dgx0 = emu_bwd(None, w_hh0, lens, g0, c0, fmt, seed=4, d_in=dgx1, w_in=w_ih1)
    valid = torch.arange(T)[:, None] < lens.long()[None, :]
    d16 = R.op16(R.on_valid(dgx1, valid), fmt)
    cb = emu_c_acc(8 * Hd, fmt, 16)
    R.check_bwd(name + " layer 0", d16 @ W, w_hh0, lens, g0, c0, dgx0, fmt, dy_tol=cb * R.U32 * (d16.abs() @ W.abs()), c_acc=cb)
    # the hand-off one step off (layer 0 reading dgates1 of the neighbouring step) is caught
    if T >= 3:
        shifted = torch.roll(d16, 1, 0) @ W
        assert R.replay_bwd(shifted, w_hh0, lens, g0, c0, dgx0, fmt, dy_tol=cb * R.U32 * (d16.abs() @ W.abs()), c_acc=cb) >= R.SHARP


def test_derived_constants():
    """the constants the GPU file passes, as the helper's docstring derives them"""
    assert [R.c_acc_of("fwd16", H) for H in (128, 640, 1024)] == [5, 9, 12]
    assert [R.c_acc_of("bwd16", H) for H in (128, 640, 1024)] == [17, 21, 24]
    assert R.c_acc_of("l2f1_in", 1024) == 20 and R.c_acc_of("l2b0_in", 768) == 28 and R.c_acc_of("l2b0_sk", 1024) == 40
    assert [R.c_acc_of("fwd32", H) for H in (16, 20, 68, 256)] == [20, 20, 36, 68]
    assert [R.c_acc_of("bwd32", H) for H in (16, 256)] == [23, 71]
    assert R.C_ACC == 16 and R.act_eps(0) < R.act_eps(1)
