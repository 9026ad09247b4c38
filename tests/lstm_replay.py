"""Step-by-step float64 replay of an LSTM recurrence (imported by the tests, not collected).  Plain torch on whatever device the
tensors live on; nothing here calls the project's kernels.

Each step is checked on its own: the previous state is taken from the kernel's OWN saved outputs, the step is recomputed in float64
with exactly the operand rounding the kernel applies (fmt 1 / 2: round-to-nearest-even to bf16 / fp16 = torch's cast; fmt 0, the
fp32 parity mode: none), and every element is compared.

  forward   z = gx + op16(W_hh) . op16(h_prev);  gates = (sigma, sigma, tanh, sigma)(z);  cell = f c_prev + i g;  y = o tanh(cell)
  backward  dh = dy + op16(W_hh)^T . op16(dgates_next);  dc = dh o (1 - tanh^2 cell) + f_next dc_next;  dgates from the saved gates

Tolerances are bounds, stated per element (u = 2^-24, the fp32 unit roundoff):
  |dz|   <= c_acc u (|gx| + sum_k |op16(W)| |op16(h)|) (+ gx_tol)
  gates  <= act'(z) |dz| + act_eps(fmt)
  cell   <= 2 u (|i g| + |cell|);  y <= |o| act_eps + 2 u |y|
  backward: the dh bound as |dz| (+ dy_tol), carried through the dc scan together with dc itself (see replay_bwd).

act_eps: 2^-20 for the v_exp_f32 / v_rcp_f32 forms (common.h lstm_cell<true> / lstm_cell_bwd<true>); 2^-22 for the exact forms of
the parity mode (lstm_cell<false>: 1 / (1 + expf(-x)) = a 1-ulp expf, one addition and one division, each at most u relative of a
value <= 1 -> 3 u, rounded up to 4 u; tanhf within 2 ulp of a value <= 1).

c_acc = the number of fp32 roundings on the longest path from a product to the pre-activation; one matrix instruction's update of
its accumulator counts as one rounding per instruction for the 16-bit MFMA 16x16x32 (the convention the persistent kernels' C_ACC =
16 was derived with and holds under), and as one (fused) rounding per k for the fp32 MFMA 16x16x4, whose four products enter the
accumulator one after the other.  The default C_ACC = 16 keeps its meaning for the persistent kernels (32 k-chunk MFMAs split over
the waves plus the fp32 sums of their partials).  The launch-per-step kernels, from csrc/lstm.hip and csrc/lstm2.hip (`c_acc_of`):

  fwd16    lstm_fwd_body<1>, lstm2 layer 0: 4 waves split H/32 chunks -> H/128 MFMAs on one accumulator; pre = red0 + red1 + red2 +
           red3 + gx: 4 additions.                                                                         H/128 + 4   (<= 12)
  bwd16    lstm_bwd_body_bf16, lstm2 layer 1: 16 waves split 4H/32 chunks -> H/128 MFMAs; dh = dy, dh += red[w] sixteen times: the
           first partial passes through all 16 additions.                                                  H/128 + 16  (<= 24)
  l2f1_in  lstm2 forward layer 1, a product of the INPUT segment (h0 . W_ih1): both K segments share one accumulator and the input
           segment goes first, so its products see the MFMAs of both segments; sum = b1, sum += red[w] four times.
                                                                                                           2 H/128 + 4 (<= 20)
  l2f1     lstm2 forward layer 1, a product of the recurrent segment (second in the accumulator): as fwd16.
  l2b0_in  lstm2_bwd_step layer 0, a product of dgates1 . W_ih1 (first segment of the shared accumulator).  2 H/128 + 16 (<= 32)
  l2b0     lstm2_bwd_step / lstm2_bwd_skew2 layer 0, a product of the recurrent segment: as bwd16.
  l2b0_sk  lstm2_bwd_skew2 layer 0, a product of dgates1 . W_ih1: 8 MFMAs in the layer-1 workgroup (accp), pv = sum of 16 partials
           (16 additions), stored as fp32; the layer-0 workgroup one launch later starts dh from it and adds its own 16 partials.
                                                                                                           8 + 16 + 16 = 40
  fwd32    lstm_fwd_body<0> (skinny_f32): ceil(H/16) chunks of 16 k over 4 waves, every k one fused rounding into the accumulator
           -> 16 ceil(ceil(H/16) / 4); then the 4 additions of fwd16.                             16 ceil(ceil(H/16)/4) + 4
  bwd32    lstm_bwd_matmul + lstm_bwd_pointwise: one of four K slices of length H per workgroup, as fwd32's chain; part_out =
           red0 + red1 + red2 + red3 (3 additions); dh = dy + part0 + part1 + part2 + part3 (4).   16 ceil(ceil(H/16)/4) + 7

Each check also proves the replay is sharp: mutations -- W_hh not rounded to 16 bits (fmt 0, inverted: W_hh rounded to bf16 where
the kernel does not), h_prev (dgates_next) taken from the neighbouring batch row, or from one step off -- must each exceed the
tolerance at least tenfold."""
import torch

U32 = 2.0 ** -24
C_ACC = 16
ACT_EPS = 2.0 ** -20
ACT_EPS_EXACT = 2.0 ** -22
SHARP = 10.0


def dt16(fmt):
    return torch.float16 if fmt == 2 else torch.bfloat16


def op16(t, fmt):
    return t.double() if fmt == 0 else t.to(dt16(fmt)).double()


def act_eps(fmt):
    return ACT_EPS_EXACT if fmt == 0 else ACT_EPS


def c_acc_of(kind, H):
    """the derived accumulation constants of the launch-per-step kernels (module docstring)"""
    per16 = -(-H // 128)
    per32 = 16 * (-(-(-(-H // 16)) // 4))
    return {"fwd16": per16 + 4, "bwd16": per16 + 16, "l2f1_in": 2 * per16 + 4, "l2f1": per16 + 4, "l2b0_in": 2 * per16 + 16,
            "l2b0": per16 + 16, "l2b0_sk": 8 + 16 + 16, "fwd32": per32 + 4, "bwd32": per32 + 7}[kind]


def steps(lens, T, reverse, off=1):
    """valid mask [T, B] and, per (t, b), the time of the step `off` steps earlier in the row's own order (clamped) with its mask"""
    t = torch.arange(T, device=lens.device)[:, None]
    ln = lens.long()[None, :]
    valid = t < ln
    tp = t + off if reverse else t - off
    has = valid & (tp >= 0) & (tp < ln)
    return valid, tp.clamp(0, T - 1).expand(T, lens.numel()), has


def gather_rows(x, tp, bidx, has=None):
    """x[tp[t, b], bidx[b]]; where `has` is False: 0 (pad rows of saved gates / cell are never written: no NaN * 0)"""
    r = x[tp, bidx[None, :].expand_as(tp)]
    return r if has is None else torch.where(has[..., None], r, torch.zeros((), dtype=r.dtype, device=r.device))


def on_valid(x, valid):
    return torch.where(valid[..., None], x, torch.zeros((), dtype=x.dtype, device=x.device))


def ratio(err, tol, mask):
    r = (err / tol)[mask]
    return float(r.max()) if r.numel() else 0.0


def _weights(w, fmt, mutate):
    if mutate != "w":
        return op16(w, fmt)
    return w.to(torch.bfloat16).double() if fmt == 0 else w.double()


def replay_fwd(gx, w, lens, y, g, c, fmt, reverse=False, mutate=None, gx_tol=None, c_acc=C_ACC):
    """max |kernel - replay| / tol of (gates, cell, y) over the valid (t, b); gx_tol: an extra per-element bound on gx (a gx the test
    derives itself)"""
    T, B, Hd = y.shape
    eps = act_eps(fmt)
    valid, tp, has = steps(lens, T, reverse, 2 if mutate == "step" else 1)
    bidx = torch.arange(B, device=y.device)
    if mutate == "row":
        bidx = (bidx + 1) % B
        has = has & gather_rows(valid, tp, bidx)
    h16 = op16(gather_rows(y, tp, bidx, has), fmt)
    W = _weights(w, fmt, mutate)
    z = gx.double() + h16 @ W.t()
    S = gx.double().abs() + h16.abs() @ W.abs().t()
    del h16
    tol_z = c_acc * U32 * S
    if gx_tol is not None:
        tol_z = tol_z + gx_tol
    del S
    zi, zf, zg, zo = z.chunk(4, -1)
    ref = torch.cat([torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)], -1)
    del z, zi, zf, zg, zo
    slope = ref * (1 - ref)
    slope[..., 2 * Hd:3 * Hd] = 1 - ref[..., 2 * Hd:3 * Hd] ** 2
    r_g = ratio((g.double() - ref).abs(), slope * tol_z + eps, valid[..., None].expand_as(ref))
    del ref, slope, tol_z
    if mutate is not None:
        return r_g, None, None
    _, tp1, has1 = steps(lens, T, reverse, 1)
    gi, gf, gg, go = on_valid(g.double(), valid).chunk(4, -1)
    c_prev = gather_rows(c, tp1, torch.arange(B, device=y.device), has1).double()
    c_ref = gf * c_prev + gi * gg
    r_c = ratio((c.double() - c_ref).abs(), 2 * U32 * ((gi * gg).abs() + c_ref.abs()) + 1e-38, valid[..., None].expand_as(c_ref))
    y_ref = go * torch.tanh(on_valid(c.double(), valid))
    r_y = ratio((y.double() - y_ref).abs(), go.abs() * eps + 2 * U32 * y_ref.abs() + 1e-38, valid[..., None].expand_as(y_ref))
    assert float(y[~valid].abs().max()) == 0.0 if bool((~valid).any()) else True, "pad rows of y must be exactly 0"
    return r_g, r_c, r_y


def replay_bwd(dy, w, lens, g, c, dgx, fmt, reverse=False, mutate=None, dy_tol=None, c_acc=C_ACC):
    """max |dgx - replay| / tol over the valid (t, b): dh from the kernel's own dgx of the row's next step, dc as a float64 scan
    carried together with its error bound
        E_t = |fA| e_dh + 2 |dh o tc| eps + u (3 |dh fA| + 2 |f_next dc_next| + |dc_t|) + f_next E_next,   fA = o (1 - tc^2)
    (the kernel: fA from the saved gates and its tanh, dc = fma(dh, fA, carry), carry = dc f); dy_tol: an extra per-element bound on dy
    (a dy the test derives itself), added into e_dh"""
    T, B, Hd = c.shape
    eps = act_eps(fmt)
    valid, tn, has = steps(lens, T, not reverse, 2 if mutate == "step" else 1)       # (the NEXT step: the previous one of the reversed order)
    bidx = torch.arange(B, device=dy.device)
    if mutate == "row":
        bidx = (bidx + 1) % B
        has = has & gather_rows(valid, tn, bidx)
    d16 = op16(gather_rows(dgx, tn, bidx, has), fmt)
    W = _weights(w, fmt, mutate)
    dyd = dy[..., :Hd].double()
    dh = dyd + d16 @ W
    e_dh = c_acc * U32 * (dyd.abs() + d16.abs() @ W.abs())
    if dy_tol is not None:
        e_dh = e_dh + dy_tol
    del d16
    _, tp1, hasp = steps(lens, T, reverse, 1)
    _, tn1, hasn = steps(lens, T, not reverse, 1)
    b0 = torch.arange(B, device=dy.device)
    gd = on_valid(g.double(), valid)
    gi, gf, gg, go = gd.chunk(4, -1)
    cd = on_valid(c.double(), valid)
    c_prev = gather_rows(cd, tp1, b0, hasp)
    tc = torch.tanh(cd)
    fA = go * (1 - tc * tc)
    f_next = gather_rows(gf, tn1, b0, hasn)
    dc = torch.zeros_like(cd)
    E = torch.zeros_like(cd)
    order = range(T) if reverse else reversed(range(T))
    vm = valid[..., None].double()
    for t in order:
        # the next step of row b in its own order: t + 1 (forward) / t - 1 (reverse); its dc sits there once computed
        tn_b = tn1[t]
        m = hasn[t][:, None].double()
        carry_t = dc[tn_b, b0] * m
        e_t = E[tn_b, b0] * m
        a, b = dh[t] * fA[t], f_next[t] * carry_t
        dct = (a + b) * vm[t]
        dc[t] = dct
        E[t] = (fA[t].abs() * e_dh[t] + 2 * (dh[t] * go[t] * tc[t]).abs() * eps + U32 * (3 * a.abs() + 2 * b.abs() + dct.abs())
                + f_next[t].abs() * e_t) * vm[t]
    ref = torch.cat([dc * gg * gi * (1 - gi), dc * c_prev * gf * (1 - gf), dc * gi * (1 - gg * gg), dh * tc * go * (1 - go)], -1)
    tol = torch.cat([(gg * gi * (1 - gi)).abs() * E, (c_prev * gf * (1 - gf)).abs() * E, (gi * (1 - gg * gg)).abs() * E,
                     (tc * go * (1 - go)).abs() * e_dh + (dh * go * (1 - go)).abs() * eps], -1) + 4 * U32 * ref.abs() + 1e-38
    r = ratio((dgx.double() - ref).abs(), tol, valid[..., None].expand_as(ref))
    if mutate is None:
        pad = ~valid
        if bool(pad.any()):
            assert float(dgx[pad].abs().max()) == 0.0, "pad rows of dgx must be exactly 0"
    return r


def sharp_muts(lens, B):
    if int(lens.max()) < 2:
        return []                                        # (T = 1: no recurrent term to mutate)
    out = ["w"]
    if B > 1:
        out.append("row")
    if int(lens.max()) >= 3:
        out.append("step")
    return out


def check_fwd(name, gx, w, lens, y, g, c, fmt, reverse=False, gx_tol=None, sharp=True, c_acc=C_ACC):
    """asserts the replay (every ratio <= 1) and the mutations (>= SHARP); returns (worst replay ratio, {mutation: ratio})"""
    rg, rc, ry = replay_fwd(gx, w, lens, y, g, c, fmt, reverse, gx_tol=gx_tol, c_acc=c_acc)
    muts = {m: replay_fwd(gx, w, lens, y, g, c, fmt, reverse, m, gx_tol=gx_tol, c_acc=c_acc)[0]
            for m in (sharp_muts(lens, y.shape[1]) if sharp else [])}
    with _cap():
        print("\n[replay fwd] %-44s gates %.3f  cell %.3f  y %.3f  of tol;  mutations %s" % (name, rg, rc, ry, {k: round(v, 1) for k, v in muts.items()}))
    assert rg <= 1.0 and rc <= 1.0 and ry <= 1.0, (name, rg, rc, ry)
    for m, v in muts.items():
        assert v >= SHARP, ("mutation %s not caught" % m, name, v)
    return max(rg, rc, ry), muts


def check_bwd(name, dy, w, lens, g, c, dgx, fmt, reverse=False, sharp=True, dy_tol=None, c_acc=C_ACC):
    """asserts the replay (ratio <= 1) and the mutations (>= SHARP); returns (replay ratio, {mutation: ratio})"""
    r = replay_bwd(dy, w, lens, g, c, dgx, fmt, reverse, dy_tol=dy_tol, c_acc=c_acc)
    muts = {m: replay_bwd(dy, w, lens, g, c, dgx, fmt, reverse, m, dy_tol=dy_tol, c_acc=c_acc)
            for m in (sharp_muts(lens, dy.shape[1]) if sharp else [])}
    with _cap():
        print("\n[replay bwd] %-44s dgates %.3f of tol;  mutations %s" % (name, r, {k: round(v, 1) for k, v in muts.items()}))
    assert r <= 1.0, (name, r)
    for m, v in muts.items():
        assert v >= SHARP, ("mutation %s not caught" % m, name, v)
    return r, muts


# ---- the printing shim: the [replay ...] lines reach the terminal also under pytest's capture ----------------------------------------
_CAPSYS = {}


class _cap:
    def __enter__(self):
        c = _CAPSYS.get("c")
        self.cm = c.disabled() if c is not None else None
        if self.cm is not None:
            self.cm.__enter__()

    def __exit__(self, *a):
        if self.cm is not None:
            self.cm.__exit__(*a)


def keep_capsys(capsys):
    """body of the test modules' autouse fixture (a fixture has to live in the module that uses it)"""
    _CAPSYS["c"] = capsys
    yield
    _CAPSYS.pop("c", None)


def make_weight(Hd, g):
    """a [4H, H] recurrent / input weight: N(0, 1) / sqrt(H), except that every 8th row and every 8th column keeps one entry in 16 (a
    different residue from row to row), scaled by 16.

    Why: the `w` mutation changes every weight by at most half an ulp of the 16-bit format, so over K dense products it moves a
    pre-activation by ~ sqrt(K) 2^-12 |w h| (fp16) while the accumulation bound grows like c_acc K 2^-24 |w h|: at K = 1024 .. 4096 and
    c_acc 24 .. 40 the two are within a factor of ten (measured on the dense weights: 4 .. 9 for the fp16 two-layer chain).  A row
    (forward) or column (backward) with K / 16 products of 16 times the size gives the same displacement against a sixteenth of the
    abs-sum the bound scales with -- the elements of those units decide the mutation, every other element is checked on dense rows,
    and every 32-wide k-chunk still holds two of the kept entries."""
    w = torch.randn(4 * Hd, Hd, generator=g) / Hd ** 0.5
    r, k = torch.arange(4 * Hd)[:, None], torch.arange(Hd)[None, :]
    rs, cs = (r % 8 == 0).expand_as(w), (k % 8 == 0).expand_as(w)
    keep = (~rs | (k % 16 == (r // 8) % 16)) & (~cs | (r % 16 == (k // 8) % 16))
    return torch.where(keep, torch.where(rs | cs, 16.0 * w, w), torch.zeros(()))


def make_inputs(T, B, Hd, seed, full=False, device="cpu"):
    """(gx, w, lens, dy): gx ~ 0.5 N(0, 1), w = make_weight, dy ~ 0.1 N(0, 1) (the inputs tests/test_lstm_replay_cpu.py proves the bounds
    and the mutations at); ragged int32 lengths that contain T and (B > 1) 1; full: every row T long"""
    g = torch.Generator().manual_seed(seed)
    gx = torch.randn(T, B, 4 * Hd, generator=g) * 0.5
    w = make_weight(Hd, g)
    dy = torch.randn(T, B, Hd, generator=g) * 0.1
    lens = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    lens[seed % B] = T
    if B > 1:
        lens[(seed + 1) % B] = 1
    if full:
        lens[:] = T
    return gx.to(device), w.to(device), lens.to(device), dy.to(device)


def bufs(T, B, Hd=1024, device="cuda"):
    """output buffers (y, gates, cell) pre-filled with 7.0: what the kernel does not write shows"""
    return (torch.full((T, B, Hd), 7.0, device=device), torch.full((T, B, 4 * Hd), 7.0, device=device),
            torch.full((T, B, Hd), 7.0, device=device))


def bwd64(dy, w, lens, g, c, fmt, round_w=True):
    """float64 backward recurrence with the kernels' operand roundings (op16 of W_hh and of each step's dgates in the recurrent
    product), step by step in the row's order: dgates [T, B, 4H]"""
    T, B = dy.shape[:2]
    Hd = c.shape[-1]
    W = op16(w, fmt) if round_w else w.double()
    vb = torch.arange(T, device=dy.device)[:, None] < lens.long()[None, :]
    gd, cd = on_valid(g.double(), vb), on_valid(c.double(), vb)
    gi, gf, gg, go = gd.chunk(4, -1)
    valid = vb.double()[..., None]
    tc = torch.tanh(cd)
    da = torch.zeros(T, B, 4 * Hd, dtype=torch.float64, device=dy.device)
    dc_next = torch.zeros(B, Hd, dtype=torch.float64, device=dy.device)
    f_next = torch.zeros_like(dc_next)
    rec = torch.zeros_like(dc_next)
    for t in reversed(range(T)):
        v = valid[t]
        dh = (dy[t].double() + rec) * v
        dc = (dh * go[t] * (1 - tc[t] ** 2) + f_next * dc_next) * v
        c_prev = cd[t - 1] if t > 0 else torch.zeros_like(dc)
        a = torch.cat([dc * gg[t] * gi[t] * (1 - gi[t]), dc * c_prev * gf[t] * (1 - gf[t]), dc * gi[t] * (1 - gg[t] ** 2),
                       dh * tc[t] * go[t] * (1 - go[t])], -1) * v
        da[t] = a
        rec = op16(a, fmt) @ W
        dc_next, f_next = dc, gf[t] * v
    return da
