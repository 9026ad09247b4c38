"""(-m gpu) The persistent LSTM recurrences replayed STEP BY STEP in float64.

Every other recurrence test compares one kernel with another kernel, or the whole sequence with a free-running reference to a loose
relative L2 (16-bit rounding differences cascade over hundreds of steps).  Here each step is checked on its own: the previous state is
taken from the kernel's OWN saved outputs, the step is recomputed in float64 with exactly the 16-bit operand rounding the kernel applies
(round-to-nearest-even, common.h pack_op16x2 / cvt_f16_bits = torch's `.to(bfloat16 / float16)`), and every element is compared.  All
steps are checked at once: one float64 GEMM for the recurrent products plus a short elementwise scan (the backward's dc carry).

  forward   z = gx + op16(W_hh) . op16(h_prev);  gates = (sigma, sigma, tanh, sigma)(z);  cell = f c_prev + i g;  y = o tanh(cell)
  backward  dh = dy + op16(W_hh)^T . op16(dgates_next);  dc = dh o (1 - tanh^2 cell) + f_next dc_next;  dgates from the saved gates

Tolerances are bounds, stated per element (u = 2^-24, the fp32 unit roundoff):
  |dz|   <= C_ACC u (|gx| + sum_k |op16(W)| |op16(h)|)     -- fp32 accumulation of the K = 1024 products (32 k-chunk MFMAs and the fp32
                                                               sums of their partials: at most C_ACC roundings on any path)
  gates  <= act'(z) |dz| + ACT_EPS                          -- the v_exp_f32 / v_rcp_f32 sigmoid / tanh forms (common.h lstm_cell FAST)
  cell   <= 2 u (|i g| + |cell|);  y <= |o| ACT_EPS + 2 u |y|
  backward: the dh bound as |dz|, carried through the dc scan together with dc itself (see replay_bwd).
Each test also proves the replay is sharp: three mutations -- W_hh not rounded to 16 bits, h_prev (dgates_next) taken from the
neighbouring batch row, or from one step off -- must each exceed the tolerance at least tenfold."""
import pytest
import torch

from lstm_replay import (ACT_EPS, C_ACC, SHARP, U32, _cap, bufs, bwd64, check_bwd, check_fwd, dt16, gather_rows, keep_capsys, on_valid, op16,
                         ratio, replay_bwd, replay_fwd, sharp_muts, steps)

pytestmark = pytest.mark.gpu
H = 1024


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    if not ops.persist_usable(torch.device("cuda", 0)):
        pytest.skip("persistent kernels not usable on this device")
    return L, ops


def make(T, B, seed, lens=None, scale=0.5, Hd=H):
    g = torch.Generator().manual_seed(seed)
    gx = (torch.randn(T, B, 4 * Hd, generator=g) * scale).cuda()
    w = (torch.randn(4 * Hd, Hd, generator=g) / Hd ** 0.5).cuda()
    if lens is None:
        lens = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
        lens[seed % B] = T
        if B > 3:
            lens[(seed + 1) % B] = 1
    return gx, w, torch.as_tensor(lens, dtype=torch.int32).cuda()


@pytest.fixture(autouse=True)
def _keep_capsys(capsys):
    yield from keep_capsys(capsys)


def clean(ops):
    assert ops.check_persist_status(), "a persistent launch timed out"


def run_fwd(ops, gx, w, lens, R, fmt, edges=None):
    T, B = gx.shape[:2]
    out = bufs(T, B)
    wimg = ops.roles_wimg(w, fmt, False)
    if edges is None:
        ops.roles_launch([ops.fwd_role(gx, lens, *out, wimg)], R, fmt, gx.device)
    else:
        st = torch.full((2, B, H), 7.0, device="cuda")
        for k in range(len(edges) - 1):
            ops.roles_launch([ops.fwd_role(gx, lens, *out, wimg, edges[k], edges[k + 1], st)], R, fmt, gx.device)
    torch.cuda.synchronize()
    clean(ops)
    return out


# ---- roles forward ----------------------------------------------------------------------------------------------------------------
FWD_CASES = [(1, 4), (7, 4), (20, 4), (32, 4), (20, 8), (40, 8), (64, 8), (7, 8), (40, 16), (100, 16), (128, 16), (32, 16)]


@pytest.mark.parametrize("B,R", FWD_CASES)
def test_roles_forward_replays_step_by_step(env, B, R):
    """one role, R = 4 / 8 / 16 rows per XCD group, partial and empty groups (B not a multiple of R, B < 8 R), ragged lengths with
    len 1 and len T"""
    L, ops = env
    T = 29
    gx, w, lens = make(T, B, 3 * B + R)
    y, g, c = run_fwd(ops, gx, w, lens, R, 1)
    check_fwd("roles fwd B %d R %d" % (B, R), gx, w, lens, y, g, c, 1)


@pytest.mark.parametrize("R,B", [(4, 32), (8, 64), (16, 100)])
def test_roles_forward_fp16_replays(env, R, B):
    """the fp16 twins: one case per R"""
    L, ops = env
    T = 23
    gx, w, lens = make(T, B, 5 * B + R)
    y, g, c = run_fwd(ops, gx, w, lens, R, 2)
    check_fwd("roles fwd fp16 B %d R %d" % (B, R), gx, w, lens, y, g, c, 2)


@pytest.mark.parametrize("R,B,edges", [(4, 32, [0, 1, 13, 14, 31]), (8, 40, [0, 1, 13, 14, 31]), (16, 100, [0, 9, 10, 31]),
                                       (8, 20, [0, 5, 20, 31])])
def test_roles_forward_windows_carry_state(env, R, B, edges):
    """time windows with carried (h, c): windows of width 1, and (lens <= 5 for a whole group of rows) a window in which every row of
    a group has already ended; the state buffer starts as garbage"""
    L, ops = env
    T = edges[-1]
    gx, w, lens = make(T, B, 11 * B + R)
    lens[:R] = torch.tensor([1, 2, 3, 5] * (R // 4), dtype=torch.int32, device="cuda")[:R]     # group 0 ends before the window [5, ..)
    lens[-1] = T
    y, g, c = run_fwd(ops, gx, w, lens, R, 1, edges)
    check_fwd("roles fwd windows %s R %d" % (edges, R), gx, w, lens, y, g, c, 1)


def test_roles_forward_single_step(env):
    L, ops = env
    gx, w, lens = make(1, 32, 3, lens=[1] * 32)
    y, g, c = run_fwd(ops, gx, w, lens, 4, 1)
    check_fwd("roles fwd T 1", gx, w, lens, y, g, c, 1)


@pytest.mark.parametrize("fmt", [1, 2])
def test_roles_forward_two_roles_and_16bit_gx(env, fmt):
    """two roles per launch with different lens (the DecoderPairFn skew: role 1 one window behind role 0), gx as 16-bit rows"""
    L, ops = env
    T, B, edges = 40, 32, [0, 7, 8, 40]
    a, b = make(T, B, 21), make(T, B, 22)
    ga, gb = a[0].to(dt16(fmt)), b[0].to(dt16(fmt))
    wa, wb = ops.roles_wimg(a[1], fmt, False), ops.roles_wimg(b[1], fmt, False)
    oa, ob = bufs(T, B), bufs(T, B)
    sa, sb = torch.zeros(2, B, H, device="cuda"), torch.zeros(2, B, H, device="cuda")
    n = len(edges) - 1
    for k in range(n + 1):
        roles = []
        if k < n:
            roles.append(ops.fwd_role(ga, a[2], *oa, wa, edges[k], edges[k + 1], sa))
        if k > 0:
            roles.append(ops.fwd_role(gb, b[2], *ob, wb, edges[k - 1], edges[k], sb))
        ops.roles_launch(roles, 8 if len(roles) == 2 else 4, fmt, ga.device)
    torch.cuda.synchronize()
    clean(ops)
    check_fwd("two roles, 16-bit gx, role 0 fmt %d" % fmt, ga, a[1], a[2], *oa, fmt)
    check_fwd("two roles, 16-bit gx, role 1 fmt %d" % fmt, gb, b[1], b[2], *ob, fmt)


# ---- roles backward / ft_lstm_persist_bwd_img -------------------------------------------------------------------------------------
def saved_fwd(ops, T, B, seed, fmt, lens=None):
    gx, w, lens = make(T, B, seed, lens)
    R = 4 if B <= 32 else 8 if B <= 64 else 16
    y, g, c = run_fwd(ops, gx, w, lens, R, fmt)
    torch.manual_seed(seed + 1)
    dy = torch.randn(T, B, H, device="cuda") * 0.1
    return gx, w, lens, y, g, c, dy


@pytest.mark.parametrize("B,R,fmt", [(1, 4, 1), (7, 4, 1), (32, 4, 1), (20, 8, 1), (64, 8, 1), (40, 16, 1), (100, 16, 1), (128, 16, 1),
                                     (32, 4, 2), (64, 8, 2), (100, 16, 2)])
def test_roles_backward_replays_step_by_step(env, B, R, fmt):
    """one role; then the same in windows with carried (dgates, dc) and carry_in -- the state buffers start as garbage"""
    L, ops = env
    T = 27
    _, w, lens, y, g, c, dy = saved_fwd(ops, T, B, 7 * B + R + fmt, fmt)
    wimg = ops.roles_wimg(w, fmt, True)
    d1 = torch.full((T, B, 4 * H), 7.0, device="cuda")
    ops.roles_launch([ops.bwd_role(dy, lens, g, c, d1, wimg)], R, fmt, dy.device, backward=True)
    torch.cuda.synchronize()
    clean(ops)
    check_bwd("roles bwd B %d R %d fmt %d" % (B, R, fmt), dy, w, lens, g, c, d1, fmt)
    d2 = torch.full((T, B, 4 * H), 7.0, device="cuda")
    st = (torch.full((B, 4 * H), 7.0, device="cuda"), torch.full((B, H), 7.0, device="cuda"))
    edges = [0, 1, 13, 14, T]
    for k in reversed(range(len(edges) - 1)):
        ops.roles_launch([ops.bwd_role(dy, lens, g, c, d2, wimg, edges[k], edges[k + 1], st, carry_in=k < len(edges) - 2)], R, fmt, dy.device,
                         backward=True)
    torch.cuda.synchronize()
    clean(ops)
    check_bwd("roles bwd windows B %d R %d fmt %d" % (B, R, fmt), dy, w, lens, g, c, d2, fmt, sharp=False)
    if B <= 32:
        # the compact image output beside the fp32 rows: op16 of the replayed rows in RowMap order, dbias a float64 column sum
        rm = ops.row_map(lens, T, B)
        img = ops.Bf16Image.empty_rows(4 * H, rm, fmt, dy.device)
        d3 = torch.full((T, B, 4 * H), 7.0, device="cuda")
        ops.roles_launch([ops.bwd_role(dy, lens, g, c, d3, wimg, dimg=img)], R, fmt, dy.device, backward=True)
        torch.cuda.synchronize()
        clean(ops)
        check_image_and_dbias(d3, img, img.colsum, lens, T, B, fmt)


def compact_rows(x, lens, T, B, cols):
    """batch-major compact rows of the valid frames of x [T, B, cols], ONE zero separator row per utterance (RowMap's order)"""
    parts = []
    for b in range(B):
        n = int(lens[b])
        parts.append(x[:n, b])
        parts.append(torch.zeros(1, cols, dtype=x.dtype, device=x.device))
    return torch.cat(parts, 0)


def image_rows(img, nrows, fmt):
    return img.buf[:nrows * img.ld * 2].view(dt16(fmt)).reshape(nrows, img.ld)[:, :img.cols]


@pytest.mark.parametrize("B,fmt", [(32, 1), (7, 1), (32, 2)])
def test_persist_bwd_img_replays_and_its_image_is_the_replayed_dgates(env, B, fmt):
    """ft_lstm_persist_bwd_img (the reduce-scatter backward, ng 21): fp32 dgates beside the image replay step by step; the compact
    image = op16 of those rows in RowMap order; dbias = a float64 column sum; the image-only call (dgx = NULL) writes the same image"""
    L, ops = env
    T = 31
    _, w, lens, y, g, c, dy = saved_fwd(ops, T, B, 13 * B + fmt, fmt)
    st = ops._persist_watch(dy.device)
    work = torch.empty(L.lib().ft_lstm_persist_workspace_bytes(B, H), device="cuda", dtype=torch.uint8)
    rm = ops.row_map(lens, T, B)
    outs = []
    for with_dgx in (True, False):
        img = ops.Bf16Image.empty_rows(4 * H, rm, fmt, dy.device)
        img.colsum.zero_()
        d = torch.full((T, B, 4 * H), 7.0, device="cuda") if with_dgx else None
        L.check(L.op16("ft_lstm_persist_bwd_img", fmt)(L.ptr(dy), H, L.ptr(w), L.ptr(lens), L.ptr(g), L.ptr(c), L.ptr(d), L.ptr(work), L.ptr(st.status),
                                                      T, B, H, 21, L.ptr(img.buf), img.ld, img.buf.numel() // (2 * img.ld), L.ptr(img.colsum), L.stream()),
                "ft_lstm_persist_bwd_img")
        ops._persist_arm(st)
        torch.cuda.synchronize()
        clean(ops)
        outs.append((d, img, img.colsum.clone()))
    (d, img, cs), (_, img0, cs0) = outs
    check_bwd("persist bwd img B %d fmt %d" % (B, fmt), dy, w, lens, g, c, d, fmt)
    check_image_and_dbias(d, img, cs, lens, T, B, fmt)
    check_image_and_dbias(d, img0, cs0, lens, T, B, fmt)          # the image-only call: the image of the same dgates


def check_image_and_dbias(d, img, cs, lens, T, B, fmt):
    n = int(lens.sum()) + B
    assert torch.equal(image_rows(img, n, fmt), compact_rows(d, lens, T, B, 4 * H).to(dt16(fmt)))
    valid = (torch.arange(T, device="cuda")[:, None] < lens[None, :])
    ref = d.double()[valid].sum(0)
    e = ((cs.double() - ref).abs() / (d.double().abs()[valid].sum(0) * 64 * U32 + 1e-38)).max()      # (fp32 atomics: 64 u of the abs sum)
    assert float(e) <= 1.0, float(e)


# ---- bidirectional pair -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [1, 2])
def test_bilstm_persist_replays_both_directions(env, fmt):
    """ft_bilstm_persist_fwd / _bwd (the encoder's pair, H 256): both directions, ragged lengths including 1 and T"""
    L, ops = env
    T, B, H = 37, 32, 256
    if not ops.bilstm_persist_ok(B, H, fmt, torch.device("cuda", 0)):
        pytest.skip("bidirectional persistent kernel not usable here")
    lens = [T, 1, 2, T - 1] + [max(1, T - 3 * i) for i in range(B - 4)]
    gf, wf, lens = make(T, B, 41 + fmt, lens, Hd=H)
    gr, wr, _ = make(T, B, 43 + fmt, lens.cpu(), Hd=H)
    y = torch.full((T, B, 2 * H), 7.0, device="cuda")
    gs = [torch.full((T, B, 4 * H), 7.0, device="cuda") for _ in range(2)]
    cs = [torch.full((T, B, H), 7.0, device="cuda") for _ in range(2)]
    st = ops._persist_watch(gf.device)
    work = torch.empty(L.lib().ft_bilstm_persist_workspace_bytes(B, H), device="cuda", dtype=torch.uint8)
    L.check(L.op16("ft_bilstm_persist_fwd", fmt)(L.ptr(gf), L.ptr(gr), L.ptr(wf), L.ptr(wr), L.ptr(lens), L.ptr(y), 2 * H, L.ptr(gs[0]), L.ptr(gs[1]),
                                                  L.ptr(cs[0]), L.ptr(cs[1]), L.ptr(work), L.ptr(st.status), T, B, H, L.stream()), "ft_bilstm_persist_fwd")
    ops._persist_arm(st, bilstm=True)
    torch.cuda.synchronize()
    clean(ops)
    yf, yr = y[..., :H].contiguous(), y[..., H:].contiguous()
    check_fwd("bilstm fwd dir 0 fmt %d" % fmt, gf, wf, lens, yf, gs[0], cs[0], fmt)
    check_fwd("bilstm fwd dir 1 fmt %d" % fmt, gr, wr, lens, yr, gs[1], cs[1], fmt, reverse=True)
    torch.manual_seed(3)
    dy = torch.randn(T, B, 2 * H, device="cuda") * 0.1
    d = [torch.full((T, B, 4 * H), 7.0, device="cuda") for _ in range(2)]
    L.check(L.op16("ft_bilstm_persist_bwd", fmt)(L.ptr(dy), 2 * H, L.ptr(wf), L.ptr(wr), L.ptr(lens), L.ptr(gs[0]), L.ptr(gs[1]), L.ptr(cs[0]),
                                                  L.ptr(cs[1]), L.ptr(d[0]), L.ptr(d[1]), L.ptr(work), L.ptr(st.status), T, B, H, L.stream()), "ft_bilstm_persist_bwd")
    ops._persist_arm(st, bilstm=True)
    torch.cuda.synchronize()
    clean(ops)
    check_bwd("bilstm bwd dir 0 fmt %d" % fmt, dy[..., :H].contiguous(), wf, lens, gs[0], cs[0], d[0], fmt)
    check_bwd("bilstm bwd dir 1 fmt %d" % fmt, dy[..., H:].contiguous(), wr, lens, gs[1], cs[1], d[1], fmt, reverse=True)


# ---- padded hidden sizes through ops.lstm_layer -----------------------------------------------------------------------------------
def seq_node(h):
    """the LSTMSeqFn node behind lstm_layer's output (through the slice / contiguous of the padded path)"""
    todo, seen = [h.grad_fn], set()
    while todo:
        n = todo.pop()
        if n is None or id(n) in seen:
            continue
        seen.add(id(n))
        if "LSTMSeqFn" in type(n).__name__:
            return n
        todo.extend(f for f, _ in n.next_functions)
    raise AssertionError("no LSTMSeqFn node")


@pytest.mark.parametrize("Hs", [512, 640, 768])
def test_padded_hidden_sizes_replay_and_padding_stays_inert(env, Hs, monkeypatch):
    """H < 1024 runs as the zero-padded 1024-unit twin: replay the 1024-wide saved tensors; a padded unit keeps gates exactly
    (0.5, 0.5, 0, 0.5) and cell / y / dgx exactly 0 -- what lstm_layer's padding argument rests on"""
    L, ops = env
    T, B, K, fmt = 70, 16, 256, 1
    monkeypatch.setattr(ops, "_PERSIST_IMG", "both")                 # fp32 dgates beside the image: the replay reads them
    dev = torch.device("cuda", 0)
    if not ops.lstm_pad_width(B, Hs, False, fmt, dev, T):
        pytest.skip("padded path not taken on this device")
    torch.manual_seed(Hs)
    x = torch.randn(T, B, K, device="cuda") * 0.5
    w_ih = (torch.randn(4 * Hs, K, device="cuda") / K ** 0.5).requires_grad_(True)
    w_hh = (torch.randn(4 * Hs, Hs, device="cuda") / Hs ** 0.5).requires_grad_(True)
    b_ih, b_hh = (torch.randn(4 * Hs, device="cuda") * 0.1).requires_grad_(True), torch.zeros(4 * Hs, device="cuda", requires_grad=True)
    lens = torch.randint(1, T + 1, (B,), dtype=torch.int32)
    lens[0], lens[1] = T, 1
    lens = lens.cuda()
    rm = ops.row_map(lens, T, B)
    h = ops.lstm_layer(x, lens, w_ih, w_hh, b_ih, b_hh, mode=fmt, rowmap=rm)
    assert h.shape[-1] == Hs
    node = seq_node(h)
    w_p, lens_s, y, g, c = node.saved_tensors
    assert w_p.shape == (4 * H, H)
    lin = node.next_functions[0][0]                                  # the input projection: its incoming gradient is the kernel's dgx
    assert lin is not None
    dgx_seen = []
    lin.register_prehook(lambda grads: dgx_seen.append(grads[0]))
    torch.manual_seed(1)
    dh = torch.randn(T, B, Hs, device="cuda") * 0.1
    h.backward(dh)
    torch.cuda.synchronize()
    clean(ops)
    valid = (torch.arange(T, device="cuda")[:, None] < lens[None, :])
    pad = slice(Hs, H)
    gv = g[valid].view(-1, 4, H)[..., pad]
    want = torch.tensor([0.5, 0.5, 0.0, 0.5], device="cuda")[None, :, None].expand_as(gv)
    assert torch.equal(gv, want), "padded units must keep gates (0.5, 0.5, 0, 0.5) exactly"
    assert float(c[valid][:, pad].abs().max()) == 0.0 and float(y[..., pad].abs().max()) == 0.0
    dgx = dgx_seen[0].float()
    assert float(dgx[valid].view(-1, 4, H)[..., pad].abs().max()) == 0.0, "padded units must get dgates exactly 0"
    # the replay: gx = the padded projection in float64 with the operands the projection GEMM rounds (the bound: its fp32 accumulation,
    # plus one 16-bit ulp where gx travels as 16-bit rows)
    w_ih_p = ops.pad_gate_blocks(w_ih.detach(), 0)
    b_p = ops.pad_gate_blocks((b_ih + b_hh).detach(), 0)
    x16 = op16(x, fmt)
    gx = b_p.double() + x16 @ op16(w_ih_p, fmt).t()
    gx_tol = C_ACC * U32 * (b_p.double().abs() + x16.abs() @ op16(w_ih_p, fmt).abs().t())
    if node.gx_dtype == torch.float32:
        gx_tol = gx_tol + U32 * gx.abs()
    else:                                                            # (16-bit rows: certain where the bound straddles no rounding midpoint)
        lo, hi = op16(gx - gx_tol, fmt), op16(gx + gx_tol, fmt)
        gx, gx_tol = (lo + hi) / 2, 1.05 * (hi - lo).abs() / 2
    check_fwd("padded H %d fwd" % Hs, gx, w_p.detach(), lens, y, g, c, fmt, gx_tol=gx_tol)
    dy = torch.zeros(T, B, H, device="cuda")
    dy[..., :Hs] = dh
    check_bwd("padded H %d bwd" % Hs, dy, w_p.detach(), lens, g, c, dgx, fmt)


# ---- the decoder pair -------------------------------------------------------------------------------------------------------------
def pair_inputs(T, B, seed, lens=None):
    g = torch.Generator().manual_seed(seed)
    gx0 = (torch.randn(T, B, 4 * H, generator=g) * 0.5).cuda()
    w_hh0, w_ih1, w_hh1 = [(torch.randn(4 * H, H, generator=g) / H ** 0.5).cuda().requires_grad_(True) for _ in range(3)]
    b_ih1, b_hh1 = [(torch.randn(4 * H, generator=g) * 0.1).cuda().requires_grad_(True) for _ in range(2)]
    if lens is None:
        lens = torch.randint(max(1, T // 3), T + 1, (B,), generator=g, dtype=torch.int32)
        lens[seed % B] = T
        lens[(seed + 1) % B] = 1
    return gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, torch.as_tensor(lens, dtype=torch.int32).cuda()


def pair_forward(ops, fmt, gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens, nch, private=False):
    T, B = gx0.shape[:2]
    rm = ops.row_map(lens, T, B)
    y1 = ops.DecoderPairFn.apply(gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens, fmt, rm, private, nch)
    torch.cuda.synchronize()
    clean(ops)
    return y1


def check_pair_forward(name, ops, fmt, gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens, y1, sharp=True):
    _, _, _, _, y0, g0, c0, y1s, g1, c1 = y1.grad_fn.saved_tensors
    assert y1s.data_ptr() == y1.data_ptr()
    check_fwd(name + " layer 0", gx0, w_hh0.detach(), lens, y0, g0, c0, fmt, sharp=sharp)
    b1 = (b_ih1 + b_hh1).detach().double()               # (fp32 sum, as bias_sum)
    y16 = op16(y0, fmt)
    W = op16(w_ih1.detach(), fmt)
    gx1 = b1 + y16 @ W.t()
    tol = C_ACC * U32 * (b1.abs() + y16.abs() @ W.abs().t())
    if gx0.dtype == torch.float32:
        gx1, tol = gx1, tol + U32 * gx1.abs()
    else:
        lo, hi = op16(gx1 - tol, fmt), op16(gx1 + tol, fmt)
        gx1, tol = (lo + hi) / 2, 1.05 * (hi - lo).abs() / 2          # (x 1.05: the activation's slope changes across one 16-bit ulp)
    check_fwd(name + " layer 1", gx1, w_hh1.detach(), lens, y1, g1, c1, fmt, gx_tol=tol, sharp=sharp)


@pytest.mark.parametrize("nch", [2, 3, 4, 6])
@pytest.mark.parametrize("g16", [False, True])
def test_decoder_pair_forward_replays_both_layers(env, nch, g16):
    """DecoderPairFn called directly: layer 0 on the test's gx0, layer 1 on gx1 = b1 + op16(W_ih1) op16(y0) in float64 -- which checks
    the per-chunk projection GEMMs and their row maps element by element (16-bit gx1 rows: within one 16-bit ulp where the GEMM's
    fp32 bound straddles a rounding midpoint, exact elsewhere)"""
    L, ops = env
    T, B, fmt = 48, 32, 1
    ins = list(pair_inputs(T, B, 60 + nch))
    if g16:
        ins[0] = ins[0].to(dt16(fmt))
    y1 = pair_forward(ops, fmt, *ins, nch)
    check_pair_forward("pair fwd nch %d gx16 %d" % (nch, g16), ops, fmt, *ins, y1)


def pair_reference_grads(fmt, w_hh0, w_ih1, w_hh1, lens, y0, g0, c0, y1, g1, c1, dy1, round_w=True):
    T, B = y1.shape[:2]
    valid = (torch.arange(T, device=y1.device)[:, None] < lens.long()[None, :])
    vm = valid.double()[..., None]
    da1 = bwd64(dy1, w_hh1, lens, g1, c1, fmt, round_w)
    d16 = op16(da1, fmt)
    y0_16, y1_16 = op16(on_valid(y0, valid), fmt), op16(on_valid(y1, valid), fmt)
    dy0 = (d16 @ op16(w_ih1, fmt)) * vm
    da0 = bwd64(dy0, w_hh0, lens, g0, c0, fmt, round_w)
    d0_16 = op16(da0, fmt)
    flat = lambda x: x.reshape(-1, x.shape[-1])
    dW_hh1 = flat(d16[1:]).t() @ flat(y1_16[:-1])
    dW_ih1 = flat(d16).t() @ flat(y0_16)
    dW_hh0 = flat(d0_16[1:]).t() @ flat(y0_16[:-1])
    db1 = flat(da1).sum(0)
    return dict(dgx0=da0, dW_hh0=dW_hh0, dW_ih1=dW_ih1, db1=db1, dW_hh1=dW_hh1)


# rel-L2 per gradient.  The pair's layer-1 dgates never leave the node, so this comparison is FREE-RUNNING over the sequence: fp32
# differences and the op16 ties they tip compound through both backward recurrences (observed 2e-4 .. 1.4e-3 at T 48 / 862; the
# unrounded-W_hh replay is only ~2x further off, so the test cannot prove sharpness here).  The step-local replays above hold the
# same kernels element by element; this one holds the pair's plumbing -- chunk windows, carried state, the dX GEMMs between launches.
PAIR_BWD_TOL = 2e-3


@pytest.mark.parametrize("nch,nch_bwd", [(4, 0), (4, -1), (4, 3), (6, 2), (2, 0), (3, -1)])
def test_decoder_pair_backward_against_float64(env, monkeypatch, nch, nch_bwd):
    """the pair's backward (dgx0, dW_hh0, dW_ih1, dW_hh1, db1) against a float64 backward with the same operand roundings, on every
    path: sequential (nch_bwd 0), the forward's chunks (-1) and a chunking of its own"""
    L, ops = env
    T, B, fmt = 48, 32, 1
    monkeypatch.setattr(ops, "_PERSIST_IMG", "both")                  # fp32 dgx0 on every path
    monkeypatch.setattr(ops, "_PAIR_CHUNKS_BWD", nch_bwd)
    gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens = pair_inputs(T, B, 90 + nch)
    gx0.requires_grad_(True)
    y1 = pair_forward(ops, fmt, gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens, nch, private=True)
    _, _, _, _, y0, g0, c0, _, g1, c1 = y1.grad_fn.saved_tensors
    torch.manual_seed(nch)
    dy1 = torch.randn(T, B, H, device="cuda") * 0.1
    y1.backward(dy1)
    torch.cuda.synchronize()
    clean(ops)
    got = dict(dgx0=gx0.grad, dW_hh0=w_hh0.grad, dW_ih1=w_ih1.grad, db1=b_ih1.grad, dW_hh1=w_hh1.grad)
    assert torch.equal(b_ih1.grad, b_hh1.grad)
    args = (fmt, w_hh0.detach(), w_ih1.detach(), w_hh1.detach(), lens, y0, g0, c0, y1.detach(), g1, c1, dy1)
    ref = pair_reference_grads(*args)
    mut = pair_reference_grads(*args, round_w=False)
    valid = (torch.arange(T, device="cuda")[:, None] < lens[None, :])[..., None]
    errs, muts = {}, {}
    for k in got:
        a = got[k].double()
        if k == "dgx0":
            a = on_valid(a, valid[..., 0])
        errs[k] = float((a - ref[k]).norm() / ref[k].norm())
        muts[k] = float((a - mut[k]).norm() / mut[k].norm())
    with _cap():
        print("\n[replay pair bwd] nch %d / %d  rel-L2 %s  tol %.0e;  W_hh unrounded %s" % (
            nch, nch_bwd, {k: "%.2e" % v for k, v in errs.items()}, PAIR_BWD_TOL, {k: "%.2e" % v for k, v in muts.items()}))
    for k, e in errs.items():
        assert e <= PAIR_BWD_TOL, (k, e)


# ---- the benchmark's shape --------------------------------------------------------------------------------------------------------
def bench_lens(B):
    import bench
    b = bench.synth_batch(B, 1234 + 7)
    return b["out_lens"].to(torch.int32)


def test_bench_shape_roles_forward_and_reduce_scatter_backward(env):
    """T 862, B 32, H 1024 with the benchmark's lengths: the roles forward (R = 4) and the reduce-scatter backward, every step"""
    L, ops = env
    B = 32
    lens = bench_lens(B)
    T = int(lens.max())
    gx, w, lens, y, g, c, dy = saved_fwd(ops, T, B, 1234, 1, lens)
    check_fwd("bench shape roles fwd", gx, w, lens, y, g, c, 1)
    del gx
    st = ops._persist_watch(dy.device)
    work = torch.empty(L.lib().ft_lstm_persist_workspace_bytes(B, H), device="cuda", dtype=torch.uint8)
    d = torch.full((T, B, 4 * H), 7.0, device="cuda")
    L.check(L.lib().ft_lstm_persist_bwd(L.ptr(dy), H, L.ptr(w), L.ptr(lens), L.ptr(g), L.ptr(c), L.ptr(d), L.ptr(work), L.ptr(st.status),
                                        T, B, H, 21, L.stream()), "ft_lstm_persist_bwd")
    ops._persist_arm(st)
    torch.cuda.synchronize()
    clean(ops)
    check_bwd("bench shape reduce-scatter bwd", dy, w, lens, g, c, d, 1)


def test_bench_shape_decoder_pair(env, monkeypatch):
    L, ops = env
    B, fmt = 32, 1
    lens = bench_lens(B)
    T = int(lens.max())
    monkeypatch.setattr(ops, "_PERSIST_IMG", "both")
    monkeypatch.setattr(ops, "_PAIR_CHUNKS_BWD", 0)
    gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens = pair_inputs(T, B, 5, lens)
    gx0.requires_grad_(True)
    y1 = pair_forward(ops, fmt, gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens, 6, private=True)
    check_pair_forward("bench shape pair fwd", ops, fmt, gx0.detach(), w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens, y1)
    _, _, _, _, y0, g0, c0, _, g1, c1 = y1.grad_fn.saved_tensors
    torch.manual_seed(0)
    dy1 = torch.randn(T, B, H, device="cuda") * 0.1
    y1.backward(dy1)
    torch.cuda.synchronize()
    clean(ops)
    ref = pair_reference_grads(fmt, w_hh0.detach(), w_ih1.detach(), w_hh1.detach(), lens, y0, g0, c0, y1.detach(), g1, c1, dy1)
    valid = (torch.arange(T, device="cuda")[:, None] < lens[None, :])[..., None]
    got = dict(dgx0=on_valid(gx0.grad.double(), valid[..., 0]), dW_hh0=w_hh0.grad, dW_ih1=w_ih1.grad, db1=b_ih1.grad, dW_hh1=w_hh1.grad)
    errs = {k: float((got[k].double() - ref[k]).norm() / ref[k].norm()) for k in got}
    with _cap():
        print("\n[replay pair bwd] bench shape  rel-L2 %s  tol %.0e" % ({k: "%.2e" % v for k, v in errs.items()}, PAIR_BWD_TOL))
    for k, e in errs.items():
        assert e <= PAIR_BWD_TOL, (k, e)


# ---- launches whose every window is empty -----------------------------------------------------------------------------------------
def test_all_empty_windows_are_refused_and_keep_the_phase(env):
    """a roles call with every window empty (t1 == t0) launches nothing: the C entries refuse it with FT_EINVAL and ops.roles_launch
    skips it without counting it in the context's phase -- the next real launches work in the right hand-off set and replay"""
    L, ops = env
    T, B, fmt = 20, 32, 1
    gx, w, lens = make(T, B, 17)
    y, g, c = bufs(T, B)
    wf, wb = ops.roles_wimg(w, fmt, False), ops.roles_wimg(w, fmt, True)
    st = torch.zeros(2, B, H, device="cuda")
    ctx = ops.roles_ctx(gx.device)
    status = ops.persist_status(gx.device)
    dy = torch.randn(T, B, H, device="cuda") * 0.1
    d = torch.full((T, B, 4 * H), 7.0, device="cuda")
    sb = (torch.zeros(B, 4 * H, device="cuda"), torch.zeros(B, H, device="cuda"))
    ef = (L.LstmFwdRole * 1)(ops.fwd_role(gx, lens, y, g, c, wf, 7, 7, st))
    eb = (L.LstmBwdRole * 1)(ops.bwd_role(dy, lens, g, c, d, wb, 7, 7, sb, carry_in=True))
    assert L.lib().ft_lstm_roles_fwd(ef, 1, 4, ctx.reset_rows, L.ptr(ctx.buf), ctx.phase[0], L.ptr(status), H, L.stream()) == -1
    assert L.lib().ft_lstm_roles_bwd(eb, 1, 4, ctx.reset_rows, L.ptr(ctx.buf), ctx.phase[1], L.ptr(status), H, L.stream()) == -1
    phase = list(ctx.phase)
    ops.roles_launch([ops.fwd_role(gx, lens, y, g, c, wf, 0, 7, st)], 4, fmt, gx.device)
    ops.roles_launch([ops.fwd_role(gx, lens, y, g, c, wf, 7, 7, st)], 4, fmt, gx.device)
    ops.roles_launch([ops.fwd_role(gx, lens, y, g, c, wf, 7, T, st)], 4, fmt, gx.device)
    assert ctx.phase[0] == phase[0] + 2
    torch.cuda.synchronize()
    clean(ops)
    check_fwd("fwd after an empty window", gx, w, lens, y, g, c, fmt)
    for t0, t1 in ((7, T), (7, 7), (0, 7)):
        ops.roles_launch([ops.bwd_role(dy, lens, g, c, d, wb, t0, t1, sb, carry_in=t1 < T)], 4, fmt, dy.device, backward=True)
    assert ctx.phase[1] == phase[1] + 2
    torch.cuda.synchronize()
    clean(ops)
    check_bwd("bwd after an empty window", dy, w, lens, g, c, d, fmt)
