"""The decoder pair's backward pipeline over the whole-sequence dgates image: ft_gemm_img's row gather of the A operand (a_rows) against
the same GEMM over an image whose rows were gathered beforehand, and DecoderPairFn's backward pipeline against the fp32-rows pipeline
it replaced, which lives on here as the yardstick (fp32_rows_pipeline)."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN16 = {1: 0x7FC0, 2: 0x7E00}          # a quiet NaN of the operand format (FT_BF16 = 1, FT_F16 = 2)
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.lib()
    return L, ops


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def _img_rows16(img):
    """the image's storage as int16 [buffer rows, ld]"""
    return img.buf.view(torch.int16).view(-1, img.ld)


# ---------------------------------------------------------------- the gather GEMM
SRC_ROWS, CAP = 700, 384


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("K,N", [(128, 128), (128, 1024), (192, 128), (192, 1024)])
def test_gather_gemm_equals_the_gemm_over_a_pregathered_image(env, fmt, K, N):
    """compact row m reads image row a_rows[m] (a random list with repeats, out of order); every image row the list does not name holds
    NaN, C is pre-filled with a sentinel: the result equals, bit for bit, that of the plain compact GEMM over the image of the gathered
    rows, and rows the map drops (and rows at or beyond *rows_dev) keep the sentinel.  B k-contiguous and k-major."""
    L, ops = env
    gen = torch.Generator().manual_seed(100 * K + N + fmt)
    src = (torch.randn(SRC_ROWS, K, generator=gen) * 0.5).cuda()
    W = (torch.randn(N, K, generator=gen) * 0.5).cuda()
    w_img = ops.Bf16Image(W, mode=fmt)                                   # [N][K]: b_kmajor = 0
    wt_img = ops.Bf16Image(W.t().contiguous(), mode=fmt)                 # [K][N]: b_kmajor = 1
    for R in (1, 127, 128, 129, 300):
        a_rows = torch.randint(0, SRC_ROWS, (CAP,), generator=gen, dtype=torch.int32)
        a_rows[R // 2] = a_rows[0]                                      # (a repeat for certain)
        rowmap = torch.randperm(CAP, generator=gen).to(torch.int32)
        rowmap[torch.rand(CAP, generator=gen) < 0.2] = -1
        rowmap[0] = 5                                                   # (at least one row is written)
        rowmap[1:][rowmap[1:] == 5] = -1
        a_dev, rm = a_rows.cuda(), types.SimpleNamespace(map=rowmap.cuda(), rows=torch.tensor([R], dtype=torch.int32).cuda(), cap=CAP)
        # the source image: rows the list does not use (its entries at or beyond R included), and the padding rows, hold NaN
        a_img = ops.Bf16Image(src, mode=fmt)
        used = torch.zeros(_img_rows16(a_img).shape[0], dtype=torch.bool)
        used[a_rows[:R].long()] = True
        _img_rows16(a_img)[(~used).cuda()] = NAN16[fmt]
        # the reference: the gathered rows as an image of their own (zero rows behind them)
        gathered = torch.zeros(CAP, K, device="cuda")
        gathered[:R] = src[a_dev[:R].long()]
        g_img = ops.Bf16Image(gathered, mode=fmt)
        for b_km, bi in ((0, w_img), (1, wt_img)):
            c_g = torch.full((CAP, N), SENTINEL, device="cuda")
            c_r = torch.full((CAP, N), SENTINEL, device="cuda")
            ops.gemm_img(a_img, 0, a_img.ptr(), bi, b_km, bi.ptr(), c_g, CAP, N, K, N, rowmap=rm, compact=1, a_rows=a_dev)
            ops.gemm_img(g_img, 0, g_img.ptr(), bi, b_km, bi.ptr(), c_r, CAP, N, K, N, rowmap=rm, compact=1)
            torch.cuda.synchronize()
            written = torch.zeros(CAP, dtype=torch.bool)
            dest = rowmap[:R]
            written[dest[dest >= 0].long()] = True
            assert torch.isfinite(c_g).all(), (R, b_km)
            assert torch.equal(c_g, c_r), (R, b_km, (c_g - c_r).abs().max().item())
            assert bool((c_g[(~written).cuda()] == SENTINEL).all()), (R, b_km)
            assert bool((c_g[written.cuda()] != SENTINEL).any()), (R, b_km)
            ref = (src[a_dev[0].long()].double() @ W.double().t())[:8]      # (the right rows, not merely equal ones: row 0 against fp64)
            assert (c_g[int(rowmap[0])][:8].double() - ref).abs().max().item() <= 0.02 * (K ** 0.5), (R, b_km)


@pytest.mark.parametrize("fmt", [1, 2])
def test_gather_is_refused_outside_the_wide_store_kernel(env, fmt):
    """a_rows with split-K, with a k-major A, or with K = 96 (not a whole number of 64-wide stages): FT_EINVAL, nothing is launched"""
    L, ops = env
    K, N = 128, 128
    src, W = torch.randn(SRC_ROWS, K, device="cuda"), torch.randn(N, K, device="cuda")
    a_img, w_img = ops.Bf16Image(src, mode=fmt), ops.Bf16Image(W, mode=fmt)
    a_dev = torch.arange(CAP, dtype=torch.int32, device="cuda")
    rm = types.SimpleNamespace(map=torch.arange(CAP, dtype=torch.int32, device="cuda"), rows=torch.tensor([100], dtype=torch.int32).cuda(), cap=CAP)
    c = torch.full((CAP, N), SENTINEL, device="cuda")
    for kw, a_km, k in ((dict(splitk=True), 0, K), (dict(), 1, K), (dict(), 0, 96)):
        with pytest.raises(RuntimeError, match=r"ft_gemm_img failed \(-1\)"):
            ops.gemm_img(a_img, a_km, a_img.ptr(), w_img, 0, w_img.ptr(), c, CAP, N, k, N, rowmap=rm, compact=1, a_rows=a_dev, **kw)
    torch.cuda.synchronize()
    assert bool((c == SENTINEL).all())
    ops.gemm_img(a_img, 0, a_img.ptr(), w_img, 0, w_img.ptr(), c, CAP, N, K, N, rowmap=rm, compact=1, a_rows=a_dev)      # (the accepted form)
    torch.cuda.synchronize()
    assert bool((c[:100] != SENTINEL).all()) and bool((c[100:] == SENTINEL).all())


def test_chunk_row_lists_against_the_row_maps(env):
    """ft_chunk_gather_rows: a chunk's valid compact rows name their rows of the whole sequence's batch-major image and go where the
    chunk's own RowMap sends them; its separators are dropped and read a valid row of the chunk"""
    L, ops = env
    T, B = 29, 6
    lens = torch.tensor([29, 1, 10, 11, 19, 7], dtype=torch.int32)
    off = torch.cumsum(lens + 1, 0) - (lens + 1)
    ld = lens.cuda()
    for t0, t1 in ((0, 10), (10, 19), (19, 29), (0, 29)):
        lk = (lens - t0).clamp(0, t1 - t0)
        cm = ops.RowMap(lk.cuda(), t1 - t0, B)
        g = ops.ChunkGather(ld, cm, T, t0, t1)
        torch.cuda.synchronize()
        R = int(cm.rows.item())
        assert R == int(lk.sum()) + B
        a_rows, gmap, cmap = g.a_rows.cpu(), g.map.cpu(), cm.map.cpu()
        valid_rows = set()
        i = 0
        for b in range(B):
            for t in range(int(lk[b])):
                assert int(a_rows[i]) == int(off[b]) + t0 + t and int(gmap[i]) == t * B + b == int(cmap[i]), (t0, b, t)
                valid_rows.add(int(a_rows[i]))
                i += 1
            i += 1
        assert i == R
        i = 0
        for b in range(B):
            i += int(lk[b])
            assert int(gmap[i]) == -1 and int(a_rows[i]) in valid_rows, (t0, b)
            if lk[b] > 0:
                assert int(a_rows[i]) == int(a_rows[i - 1])
            i += 1


# ---------------------------------------------------------------- the pipeline branch against the fp32-rows pipeline
T_PIPE, FWD_CHUNKS = 29, 4


def _edges(T, n):
    return [(k * T + n // 2) // n for k in range(n + 1)]


def _pipe_lens(B, n):
    """lengths with 1, a chunk edge, edge + 1 and T; at B = 32 the rows 8-23 (two groups of 8 rows, four of 4) end at or before the last
    chunk's first step"""
    T = T_PIPE
    e = _edges(T, n)
    last = e[n - 1]
    if B == 5:
        return torch.tensor([e[1], 1, T, e[1] + 1, last], dtype=torch.int32)
    head = [T, 1, e[1], e[1] + 1, last, last + 1, T - 1, 2]
    mid = [last, e[1], 1, min(e[1] + 1, last), 3, 5, last - 1, 4, 1, 2, e[1], e[1] - 1, 6, min(e[1] + 1, last), last, 3]
    tail = torch.randint(1, T + 1, (8,), generator=torch.Generator().manual_seed(B + n)).tolist()
    return torch.tensor(head + mid + tail, dtype=torch.int32)


_PIPE_MODEL = {}


def _pipe_setup(B):
    import torch.nn as nn
    if "p" not in _PIPE_MODEL:
        torch.manual_seed(11)
        _PIPE_MODEL["p"] = nn.LSTM(128, 1024, 2).cuda()
    gen = torch.Generator().manual_seed(B)
    return (_PIPE_MODEL["p"], (torch.randn(T_PIPE, B, 128, generator=gen) * 0.3).cuda(), (torch.randn(T_PIPE, B, 1024, generator=gen) * 0.1).cuda())


def fp32_rows_pipeline(L, ops, saved, dy1, rm, n, mode):
    """The pair's backward as the library ran it before the pipeline over one dgates image, from the public primitives -- the yardstick:
    layer 1's dgates as fp32 rows (dgx1), one image pass per chunk over the chunk's own RowMap in front of its dX GEMM, zeroed carried
    state, layer 0's dgates as fp32 rows beside its whole-sequence image, and a second whole-sequence image (of dgx1, with the column
    sums) for the weight gradients.  `saved`: the tensors DecoderPairFn.forward saved."""
    w_hh0, w_ih1, w_hh1, lens, y0, g0, c0, y1, g1, c1 = saved
    T, B, H = y1.shape
    H4, dev = 4 * H, dy1.device
    f = dict(device=dev, dtype=torch.float32)
    edges = _edges(T, n)
    rms = [ops.RowMap((lens - a).clamp(0, b - a).to(torch.int32), b - a, B) for a, b in zip(edges, edges[1:])]
    w_img = ops.Bf16Image(w_ih1, mode=mode)
    dgx1, dgx0, dy0 = torch.empty(T, B, H4, **f), torch.empty(T, B, H4, **f), torch.empty(T, B, H, **f)
    d_img0 = ops.Bf16Image.empty_rows(H4, rm, mode, dev)
    sb1 = (torch.zeros(B, H4, **f), torch.zeros(B, H, **f))
    sb0 = (torch.zeros(B, H4, **f), torch.zeros(B, H, **f))
    wb0, wb1 = ops.roles_wimg(w_hh0, mode, True), ops.roles_wimg(w_hh1, mode, True)
    for j in range(n + 1):
        c = n - 1 - j                                        # layer 1's chunk in this launch; layer 0 runs chunk c + 1
        roles = []
        if j < n:
            roles.append(ops.bwd_role(dy1, lens, g1, c1, dgx1, wb1, edges[c], edges[c + 1], sb1, carry_in=c < n - 1))
        if j > 0:
            roles.append(ops.bwd_role(dy0, lens, g0, c0, dgx0, wb0, edges[c + 1], edges[c + 2], sb0, carry_in=c + 1 < n - 1, dimg=d_img0))
        ops.roles_launch(roles, 8 if len(roles) == 2 else 4, mode, dev, backward=True)
        if j < n:
            a, b = edges[c], edges[c + 1]
            d_img = ops.Bf16Image(dgx1[a:b].reshape((b - a) * B, H4), mode=mode, rowmap=rms[c])
            ops.gemm_img(d_img, 0, d_img.ptr(), w_img, 1, w_img.ptr(), dy0[a:b], rms[c].cap, H, H4, H, rowmap=rms[c], compact=1)
    d_img1 = ops.Bf16Image(dgx1.reshape(T * B, H4), colsum=True, mode=mode, rowmap=rm)
    y0_img, y1_img = ops.Bf16Image(y0.reshape(T * B, H), mode=mode, rowmap=rm), ops.Bf16Image(y1.reshape(T * B, H), mode=mode, rowmap=rm)
    dW_hh1, dW_ih1, dW_hh0 = torch.zeros_like(w_hh1), torch.zeros_like(w_ih1), torch.zeros_like(w_hh0)
    kw = dict(beta=1.0, splitk=True, rowmap=rm, compact=2)
    ops.gemm_img(d_img1, 1, d_img1.ptr(1), y1_img, 1, y1_img.ptr(0), dW_hh1, H4, H, rm.cap, H, k_shift=1, **kw)
    ops.gemm_img(d_img1, 1, d_img1.ptr(), y0_img, 1, y0_img.ptr(), dW_ih1, H4, H, rm.cap, H, **kw)
    ops.gemm_img(d_img0, 1, d_img0.ptr(1), y0_img, 1, y0_img.ptr(0), dW_hh0, H4, H, rm.cap, H, k_shift=1, **kw)
    torch.cuda.synchronize()
    ops.check_persist_status()
    assert torch.isfinite(dgx0).all()
    return {"weight_hh_l0": dW_hh0, "weight_ih_l1": dW_ih1, "weight_hh_l1": dW_hh1, "bias_ih_l1": d_img1.colsum, "bias_hh_l1": d_img1.colsum,
            "dgx0 image": d_img0}


@pytest.mark.parametrize("nch_bwd", [2, 3, -1])
@pytest.mark.parametrize("B", [32, 5])
def test_image_pipeline_equals_the_fp32_rows_pipeline(env, monkeypatch, B, nch_bwd):
    """DecoderPairFn.backward over `nch_bwd` windows -- both layers' dgates as whole-sequence images, each chunk's dX rows gathered out of
    layer 1's -- against the fp32-rows pipeline it replaced (fp32_rows_pipeline above, on the tensors the node's forward saved): dgx0's
    image, dW_hh0, dW_ih1 and dW_hh1 bit for bit; the bias gradient (fp32 atomics) to 1e-6.  And the node in image mode against itself
    with FLOWTRON_LSTM_PERSIST_IMG=both (the same pipeline, fp32 rows of dgx0 beside the image): those and the input projection's
    gradients made from dgx0 on the same terms.  The allocator is filled with NaN before each run: a read of an image row (or of a
    carried state) nobody wrote would show."""
    L, ops = env
    T = T_PIPE
    dev = torch.device("cuda", torch.cuda.current_device())
    assert ops.lstm_persist_groups(B, 1024, False, L.FT_BF16, dev), "persistent recurrences not usable on this device"
    n = FWD_CHUNKS if nch_bwd < 0 else nch_bwd
    lens = _pipe_lens(B, n).cuda()
    p, x0, dh = _pipe_setup(B)
    monkeypatch.setattr(ops, "_PAIR_CHUNKS_BWD", nch_bwd)
    monkeypatch.setattr(ops, "_GX16", False)                          # (gx as fp32 rows in both modes: bitwise comparison)
    taken = []
    real_branch = ops._pair_backward_pipeline
    monkeypatch.setattr(ops, "_pair_backward_pipeline", lambda *a: (taken.append(a[4]), real_branch(*a))[1])
    imgs = []
    for name in ("_handoff_put", "_handoff_put_image_only"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda t, img, *a, real=real, **kw: (imgs.append(img), real(t, img, *a, **kw))[1])
    R = int(lens.sum().item()) + B

    def image_rows(img):
        Rz = min((R + 32 + 255) // 256 * 256, _img_rows16(img).shape[0])
        return _img_rows16(img)[:Rz, :4096].clone()

    def run(img_mode):
        monkeypatch.setattr(ops, "_PERSIST_IMG", img_mode)
        del imgs[:]
        torch.empty(64 << 20, device="cuda").fill_(float("nan"))
        x = x0.clone().requires_grad_(True)
        rm = ops.row_map(lens, T, B)
        h, _ = ops.decoder_pair(x, lens, p, L.FT_BF16, [], rm, "dx", None, FWD_CHUNKS)
        saved = h.grad_fn.saved_tensors
        h.backward(dh)
        torch.cuda.synchronize()
        ops.check_persist_status()
        out = {k: q.grad.clone() for k, q in p.named_parameters()}
        out["x"] = x.grad.clone()
        for q in p.parameters():
            q.grad = None
        d_img0 = list({id(i): i for i in imgs if i.cols == 4096 and i.rowmap is rm}.values())     # (one hand-off helper calls the other)
        assert len(d_img0) == 1
        out["dgx0 image"] = image_rows(d_img0[0])
        return out, saved, rm

    both, _, _ = run("both")
    new, saved, rm = run("1")
    assert taken == [n, n], "the image pipeline runs in both modes, over %d windows: %s" % (n, taken)
    assert bool((new["dgx0 image"][: int(lens[0])] != 0).any())
    torch.empty(64 << 20, device="cuda").fill_(float("nan"))
    old = fp32_rows_pipeline(L, ops, saved, dh, rm, n, L.FT_BF16)
    old["dgx0 image"] = image_rows(old["dgx0 image"])
    for ref in (old, both):
        for k in ref:
            assert torch.isfinite(ref[k].float()).all() and torch.isfinite(new[k].float()).all(), k
            if "bias" in k:
                assert rel(new[k], ref[k]) <= 1e-6, (k, rel(new[k], ref[k]))
            else:
                assert torch.equal(new[k], ref[k]), (k, rel(new[k], ref[k]))
