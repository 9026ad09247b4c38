"""(-m gpu) The persistent forward recurrence that computes its K <= 128 input projection inside its bursts (csrc/lstm_roles.hip, the XP
kernels; ops.LSTMProjSeqFn) against the two-kernel path it replaces: ft_gemm_img with FT_GEMM_C16 writes gx as 16-bit rows, a gx16 role
reads them.

The burst forms every gx value with the GEMM's own sum (one accumulator per output, one 16x16x32 MFMA per 32 k in ascending k, the same
operand lane for every k), adds the bias in fp32 and rounds with the GEMM's converter, so y, gates and cell must be EQUAL, bit for bit
(torch.equal; the output buffers start at 7.0 on both sides, so what neither kernel writes is equal too).  Each case also replays the new
path's outputs step by step in float64 (tests/lstm_replay.py, the tolerance of the 16-bit forward kernels) on the reference's gx rows.

Shapes: H is fixed at 1024 by the kernel; T, B and K are the smallest that reach every path -- a full burst and a short one (64 + 6 steps
at R = 4, 32 + 3 at R = 8), a group with one live row and groups with none, K = 8 (one lane group of one k-step), K = 80 (a partial third
k-step), K = 128 (the bound), carried state across a window edge that is no burst edge."""
import pytest
import torch

from lstm_replay import bufs, check_fwd, dt16, keep_capsys, make_weight

pytestmark = pytest.mark.gpu
H = 1024
EINVAL = -1


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    if not ops.persist_usable(torch.device("cuda", 0)):
        pytest.skip("persistent kernels not usable on this device")
    return L, ops


@pytest.fixture(autouse=True)
def _keep_capsys(capsys):
    yield from keep_capsys(capsys)


def clean(ops):
    assert ops.check_persist_status(), "a persistent launch timed out"


def make(T, B, K, seed, lens):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, K, generator=g).cuda()
    w_ih = (torch.randn(4 * H, K, generator=g) / K ** 0.5 * 0.5).cuda()
    bias = (torch.randn(4 * H, generator=g) * 0.1).cuda()
    w_hh = make_weight(H, g).cuda()                  # (the weights tests/lstm_replay.py proves its mutations at)
    return x, w_ih, bias, w_hh, torch.as_tensor(lens, dtype=torch.int32).cuda()


def images(ops, x, w_ih, lens, fmt):
    T, B, K = x.shape
    rm = ops.RowMap(lens, T, B)
    return rm, ops.Bf16Image(x.reshape(T * B, K), mode=fmt, rowmap=rm), ops.Bf16Image(w_ih, mode=fmt)


def poison_pad(img):
    """every column beyond the image's logical width: NaN payloads (0x7FC1 is a NaN in bf16 and in fp16)"""
    v = img.buf.view(torch.int16).view(-1, img.ld)
    v[:, img.cols:] = 0x7FC1


def reference(ops, x, w_ih, bias, w_hh, lens, R, fmt, edges):
    """today's path: the projection GEMM writes 16-bit gx rows, a gx16 role reads them"""
    T, B, K = x.shape
    rm, x_img, w_img = images(ops, x, w_ih, lens, fmt)
    gx = torch.zeros(T, B, 4 * H, device="cuda", dtype=dt16(fmt))
    ops.gemm_img(x_img, 0, x_img.ptr(), w_img, 0, w_img.ptr(), gx, rm.cap, 4 * H, K, 4 * H, bias=bias, rowmap=rm, compact=1, c16=True)
    out = bufs(T, B)
    wimg = ops.roles_wimg(w_hh, fmt, False)
    st = torch.full((2, B, H), 7.0, device="cuda")
    for a, b in zip(edges, edges[1:]):
        ops.roles_launch([ops.fwd_role(gx, lens, *out, wimg, a, b, st)], R, fmt, x.device)
    return gx, out


def computed(ops, x, w_ih, bias, w_hh, lens, R, fmt, edges, poison=False):
    T, B, K = x.shape
    rm, x_img, w_img = images(ops, x, w_ih, lens, fmt)
    if poison:
        poison_pad(x_img)
        poison_pad(w_img)
    out = bufs(T, B)
    wimg = ops.roles_wimg(w_hh, fmt, False)
    st = torch.full((2, B, H), 7.0, device="cuda")
    for a, b in zip(edges, edges[1:]):
        ops.roles_launch([ops.fwd_role(None, lens, *out, wimg, a, b, st, xproj=(x_img, w_img, bias))], R, fmt, x.device)
    return out


def compare(name, ops, T, B, K, R, fmt, lens, seed, edges=None, poison=False, sharp=True):
    ins = make(T, B, K, seed, lens)
    edges = [0, T] if edges is None else edges
    gx, ref = reference(ops, *ins, R, fmt, [0, T])
    new = computed(ops, *ins, R, fmt, edges, poison)
    torch.cuda.synchronize()
    clean(ops)
    for what, a, b in zip(("y", "gates", "cell"), new, ref):
        assert torch.equal(a, b), (name, what, float((a - b).abs().max()))
    check_fwd(name, gx, ins[3], ins[4], *new, fmt, sharp=sharp)


RAGGED5 = [1, 64, 65, 70, 33]


def test_ragged_full_burst_then_short_burst(env):
    """R = 4, T = 70, B = 5: bursts of 64 and 6 steps; group 0 has four live rows (1, 64, 65, 70), group 1 one, groups 2-7 none"""
    L, ops = env
    compare("xproj R 4 T 70 B 5 K 80", ops, 70, 5, 80, 4, 1, RAGGED5, 31)


def test_fp16_build(env):
    L, ops = env
    compare("xproj fp16 R 4 T 70 B 5 K 80", ops, 70, 5, 80, 4, 2, RAGGED5, 32)


def test_smallest_k_reads_no_pad_column(env):
    """K = 8: only the lanes of k-group 0 hold values.  The pad columns [8, 256) of both images are NaN in the computed path (the reference
    multiplies clean images): equal results prove no pad column is read"""
    L, ops = env
    compare("xproj K 8 poisoned pads", ops, 9, 1, 8, 4, 1, [9], 33, poison=True, sharp=False)      # (nine steps of one row: too few elements for the mutations)


def test_k_at_its_bound_every_group_full(env):
    L, ops = env
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(1, 41, (32,), generator=g).tolist()
    lens[3], lens[4] = 40, 1
    compare("xproj R 4 T 40 B 32 K 128", ops, 40, 32, 128, 4, 1, lens, 34)


def test_eight_rows_per_group_two_bursts(env):
    """R = 8: SB = 32 steps, T = 35 is a full burst and a 3-step one; B = 40 = five full groups"""
    L, ops = env
    g = torch.Generator().manual_seed(6)
    lens = torch.randint(1, 36, (40,), generator=g).tolist()
    lens[0], lens[9], lens[39] = 35, 1, 33
    compare("xproj R 8 T 35 B 40 K 80", ops, 35, 40, 80, 8, 1, lens, 35)


def test_two_windows_carry_state(env):
    """[0, 33) then [33, 70) with carried (h, c) equals one launch: the second window's bursts start at step 33 of the image rows"""
    L, ops = env
    compare("xproj windows [0, 33, 70]", ops, 70, 5, 80, 4, 1, RAGGED5, 36, edges=[0, 33, 70])


def test_launcher_refusals(env):
    """K = 136, K = 12, a misaligned image pointer, R = 16 and mixed projection modes in one launch: FT_EINVAL, nothing launched (the
    context's phase is not advanced by the caller, and the launches after it replay)"""
    L, ops = env
    T, B, K, fmt = 12, 8, 80, 1
    x, w_ih, bias, w_hh, lens = make(T, B, K, 37, [12, 1, 5, 12, 7, 3, 12, 9])
    rm, x_img, w_img = images(ops, x, w_ih, lens, fmt)
    y, g, c = bufs(T, B)
    wimg = ops.roles_wimg(w_hh, fmt, False)
    ctx, status = ops.roles_ctx(x.device), ops.persist_status(x.device)
    gx16 = torch.zeros(T, B, 4 * H, device="cuda", dtype=dt16(fmt))

    def call(roles, R):
        arr = (L.LstmFwdRole * len(roles))(*roles)
        return L.lib().ft_lstm_roles_fwd(arr, len(roles), R, ctx.reset_rows, L.ptr(ctx.buf), ctx.phase[0], L.ptr(status), H, L.stream())

    def role(**over):
        r = ops.fwd_role(None, lens, y, g, c, wimg, xproj=(x_img, w_img, bias))
        for k, v in over.items():
            setattr(r, k, v)
        return r

    assert call([role(xproj_k=136)], 4) == EINVAL
    assert call([role(xproj_k=12)], 4) == EINVAL
    assert call([role(x_img=x_img.ptr() + 2)], 4) == EINVAL
    assert call([role(wih_img=w_img.ptr() + 8)], 4) == EINVAL
    assert call([role()], 16) == EINVAL
    half = ops.fwd_role(gx16[:, :4].contiguous(), lens[:4].contiguous(), y, g, c, wimg, nb=4)
    assert call([role(B=4), half], 8) == EINVAL
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(g.min()) == 7.0, "a refused call launched"
    compare("xproj after refusals", ops, T, B, K, 4, fmt, lens.tolist(), 37)


# ---- autograd: ops.lstm_layer on the new node against the two nodes it replaces ------------------------------------------------------
def layer_run(ops, monkeypatch, on, ins, dyw):
    x, w_ih, b_ih, b_hh, w_hh, lens = ins
    monkeypatch.setattr(ops, "_XPROJ", on)
    leaves = [t.clone().requires_grad_(True) for t in (x, w_ih, w_hh, b_ih, b_hh)]
    T, B = x.shape[:2]
    rm = ops.row_map(lens, T, B)
    y = ops.lstm_layer(leaves[0], lens, leaves[1], leaves[2], leaves[3], leaves[4], mode=1, rowmap=rm, fill="dx")
    (y * dyw).sum().backward()
    torch.cuda.synchronize()
    clean(ops)
    return [y.detach()] + [t.grad for t in leaves]


def test_lstm_layer_gradients_match_the_two_node_path(env, monkeypatch):
    """lstm_layer on [T = 70, B = 5, 80] with a RowMap and fill = "dx": the output and dx equal those of the two-node path
    (ops._XPROJ = False selects it).  dW_ih and dW_hh come from split-K GEMMs whose fp32 atomics may arrive in another order from run to
    run, and so do the bias gradients: they are the dgates image's column sums, which the backward recurrence adds up with one fp32
    atomic per batch row, five per column here (the same kernel on equal inputs in both paths; with torch.equal the new path missed one
    run of the two-node path by 2.4e-7 in db).  For these four the new path must lie as close to SOME run of the two-node path as six runs of that path lie to one
    another -- which is equality wherever that path is deterministic."""
    L, ops = env
    T, B, K = 70, 5, 80
    x, w_ih, bias, w_hh, lens = make(T, B, K, 41, RAGGED5)
    ins = (x, w_ih, bias, bias.flip(0).contiguous(), w_hh, lens)
    assert ops.xproj_ok(1, ops.row_map(lens, T, B), T, B, H, False, [x], 4 * H, None, x.device), "the case must take the new path"
    dyw = torch.randn(T, B, H, generator=torch.Generator().manual_seed(42)).cuda() * 0.1
    cur = [layer_run(ops, monkeypatch, False, ins, dyw) for _ in range(6)]
    launches = ops.PERSIST_LAUNCHES
    new = layer_run(ops, monkeypatch, True, ins, dyw)
    assert ops.PERSIST_LAUNCHES - launches == 2, "one forward and one backward persistent launch, as on the two-node path"
    for i, what in ((0, "y"), (1, "dx")):
        assert torch.equal(new[i], cur[0][i]), (what, float((new[i] - cur[0][i]).abs().max()))
    valid = (torch.arange(T, device="cuda")[:, None] < lens[None, :])
    assert float(new[1][~valid].abs().max()) == 0.0, 'fill = "dx": input-gradient rows of padded frames are zero'
    assert torch.equal(new[4], new[5]), "b_ih and b_hh receive the same gradient"
    for i, what in ((2, "dW_ih"), (3, "dW_hh"), (4, "db_ih"), (5, "db_hh")):
        spread = max(float((cur[a][i] - cur[b][i]).abs().max()) for a in range(6) for b in range(a))
        near = min(float((new[i] - r[i]).abs().max()) for r in cur)
        print("%s: two-node runs differ by %.3e, new path from the nearest of them by %.3e" % (what, spread, near))
        assert near <= spread, (what, near, spread)
