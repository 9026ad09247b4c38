"""tests/elementwise_ref64.py checked on its own, without a GPU: the exact class is exact under every emulated fp32 order and split at every
shape tests/test_gpu_elementwise_f64.py uses for it, the bounded class stays inside its bound under the same emulations (the largest
|err| / bound per operation is printed), every wrong reference of MUTATIONS is at least SHARP bounds away (exact class: unequal) at a case
the GPU file runs, and the index restatements agree with cases written out by hand."""
import pytest
import torch

import elementwise_ref64 as R
import test_gpu_elementwise_f64 as G

F32 = torch.float32
f32 = lambda v: torch.tensor(v, dtype=F32)


def split_sum(t32, order, chunk, split, seed=0):
    """rows in chunks of `chunk` (row slabs / workgroups), each summed in `order`, the partials added forward, reversed or shuffled"""
    parts = [R.emu_sum(t32[i:i + chunk], order) for i in range(0, t32.shape[0], chunk)]
    idx = list(range(len(parts)))
    if split == "rev":
        idx = idx[::-1]
    elif split == "shuffle":
        idx = torch.randperm(len(idx), generator=R.gen(seed)).tolist()
    acc = torch.zeros(t32.shape[1:], dtype=F32)
    for i in idx:
        acc = acc + parts[i]
    return acc


def every_order(t32, chunks=(32, 256)):
    """every emulated sum over dim 0 of t32: the five orders, and the three splits of each chunking"""
    for o in R.ORDERS:
        yield "order " + o, R.emu_sum(t32, o)
    for c in chunks:
        for s in R.SPLITS:
            for o in ("seq", "lanes4", "lanes16"):
                yield "chunk %d %s %s" % (c, s, o), split_sum(t32, o, c, s)


def flat_orders(t32):
    """the same for a full reduction to a scalar of a [rows, cols] term matrix, plus the grid-stride shape"""
    for tag, v in every_order(t32):
        for o in ("seq", "lanes64", "rev"):
            yield tag + " / " + o, R.emu_sum(v, o)
    for threads in (1024, 65536):
        for s in R.SPLITS:
            yield "grid-stride %d %s" % (threads, s), R.emu_flat_sum(t32, threads=threads, split=s)


def masked_terms(buf, M, lens, T, B, square):
    X = buf[:, :M]
    m = R.frame_mask(torch.as_tensor(lens, dtype=torch.int32), T).reshape(T * B, 1)
    return (X * X if square else X) * m


# ------------------------------------------------------------------------------------------------------------ exact class
MSUM_ALL = [(T, B, M, ld, lens) for T, B, M, ld, lens in G.MSUM_CASES] + [G.PASS2_SUMS + (2 * G.PASS2_SUMS[2], None)]


@pytest.mark.parametrize("T,B,M,ld,lens", MSUM_ALL)
def test_exact_masked_sum_in_any_order(T, B, M, ld, lens):
    lens = G.full_lens(T, B, 5) if lens is None else torch.tensor(lens, dtype=torch.int32)
    buf = G.msum_inputs(T, B, M, ld, "exact")
    for square in (0, 1):
        R.assert_exact((buf[:, :M].double() ** (2 if square else 1)).abs().sum(), 1.0, buf)
        ref = R.masked_sum(buf, M, lens, square, T, B)[0].float()
        for tag, got in flat_orders(masked_terms(buf, M, lens, T, B, square)):
            assert torch.equal(got, ref), (tag, square)


def test_exact_class_refuses_an_inexact_case():
    with pytest.raises(AssertionError):
        R.assert_exact(2.0 ** 24, 1.0)
    with pytest.raises(AssertionError):
        R.assert_exact(10.0, 1.0, torch.tensor([0.5]))
    R.assert_exact(10.0, 0.5, torch.tensor([0.5]))


@pytest.mark.parametrize("T,B,M,n_ls", [c[:4] for c in G.LOSS_CASES] + [G.PASS2_SUMS + (2,)])
def test_exact_loss_sums_in_any_order(T, B, M, n_ls):
    lens = G.full_lens(T, B, 8) if (T, B, M) == G.PASS2_SUMS else torch.tensor(G.LOSS_CASES[0][6], dtype=torch.int32)
    z, lsbuf, gate, target = G.loss_inputs(T, B, M, n_ls, "exact")
    views = [b[..., :M] for b in lsbuf]
    fw = R.flowtron_loss_fwd(z, views, None, None, lens, G.LOSS_SIGMA)
    m = R.frame_mask(lens, T)[:, :, None]
    z2 = (z * z * m).reshape(T * B, M)
    sl = torch.zeros(T, B, M)
    for v in views:
        sl = sl + v * m
    for tag, got in flat_orders(z2):
        assert torch.equal(got, fw["acc0"][0].float()), tag
    for tag, got in flat_orders(sl.reshape(T * B, M)):
        assert torch.equal(got, fw["acc1"][0].float()), tag
    n = R.emu_sum(lens.clamp(0, T).float(), "seq")
    assert float(n) == float(fw["acc6"][0])


@pytest.mark.parametrize("rows,N,ld", G.COLSUM_CASES)
def test_exact_colsum_in_any_order(rows, N, ld):
    buf = R.ints((max(rows, 1), ld), 1)
    ref = R.colsum(buf[:rows, :N])[0].float()
    for tag, got in every_order(buf[:rows, :N]):
        assert torch.equal(got, ref), tag


def test_exact_embedding_col2im_dbeta_and_mean_in_any_order():
    for n, dim, ld, vocab in G.EMB_CASES + [G.PASS2_EMB[:2] + (G.PASS2_EMB[1], G.PASS2_EMB[2])]:
        ids = torch.randint(0, vocab, (n,), generator=R.gen(3))
        dob = R.ints((n, ld), 5)
        ref = R.embedding_bwd(ids, dob[:, :dim], vocab)[0].float()
        for v in range(0, vocab, 7):
            for tag, got in every_order(dob[ids == v][:, :dim]):
                assert torch.equal(got, ref[v]), (tag, n, dim)
    for n, dim, stride, kind in G.RUNS_CASES:
        ids = G.runs_ids(n, stride, kind, 7)
        dob = R.ints((n, dim + 2), 6)
        ref = R.embedding_bwd(ids, dob[:, :dim], 7, stride=stride)[0].float()
        for tag, got in every_order(dob[ids == 3][:, :dim], chunks=(32,)):
            assert torch.equal(got, ref[3]), (tag, n, dim)
    for Ln, B, C, KW, lens in G.IM2COL_CASES:
        dcol = R.ints((Ln, B, C * KW), 2)
        ref = R.col2im(dcol, torch.tensor(lens, dtype=torch.int32), C, KW)[0].float()
        pad = torch.zeros(KW // 2, B, C * KW)
        wide = torch.cat([pad, dcol, pad]).reshape(Ln + 2 * (KW // 2), B, C, KW)
        terms = torch.stack([wide[KW - 1 - k:KW - 1 - k + Ln, :, :, k] for k in range(KW)])      # row l - k + KW / 2 of dcol
        m = R.frame_mask(torch.tensor(lens, dtype=torch.int32), Ln)[:, :, None]
        for o in ("seq", "rev", "lanes4"):
            assert torch.equal(R.emu_sum(terms, o) * m, ref), (o, C, KW)
    for C, keep, mis, lens, cls in G.INORM_CASES:
        if cls != "exact":
            continue
        x, gamma, beta, k, l32, dy = G.inorm_inputs(C, keep, lens, cls)
        fw = R.instnorm_fwd(x, gamma, beta, k, l32, G.INORM_EPS)
        y32 = fw["y"][0].float()
        bw = R.instnorm_bwd(x, y32, dy, gamma, k, l32, fw["mean"][0].float(), fw["rstd"][0].float())
        g = torch.where(y32 > 0, dy, torch.zeros(())) * k
        for lanes in ("lanes4", "lanes16", "seq", "rev"):
            per = [R.emu_sum(g[:min(int(l32[b]), G.INORM_L), b], lanes) for b in range(G.INORM_B)]
            for order in (range(G.INORM_B), reversed(range(G.INORM_B))):
                acc = torch.zeros(C)
                for b in order:
                    acc = acc + per[b]
                assert torch.equal(acc, bw["dbeta"][0].float())
            for b in range(G.INORM_B):
                n = min(int(l32[b]), G.INORM_L)
                if n & (n - 1) == 0:
                    s = R.emu_sum(x[:n, b], lanes)
                    assert torch.equal(s / n, fw["mean"][0][b].float()) and torch.equal(s * (f32(1.0) / n), fw["mean"][0][b].float())


# ------------------------------------------------------------------------------------------------------------ bounded class, fp32 emulations
def emu_instnorm_fwd(x, gamma, beta, keep, lens, eps, lanes):
    L, B, C = x.shape
    order = "lanes%d" % lanes
    y, mean, rstd = torch.zeros(L, B, C), torch.zeros(B, C), torch.zeros(B, C)
    for b in range(B):
        n = min(int(lens[b]), L)
        if n == 0:
            continue
        xb = x[:n, b]
        mu = R.emu_sum(xb, order) * (f32(1.0) / n) if lanes == 16 else R.emu_sum(xb, order) / n
        dd = xb - mu
        var = R.emu_sum(dd * dd, order) * (f32(1.0) / n) if lanes == 16 else R.emu_sum(dd * dd, order) / n
        rs = 1.0 / torch.sqrt(var + f32(eps))
        v = (dd * rs * gamma + beta).clamp(min=0)
        y[:n, b] = v * keep[:n, b] if keep is not None else v
        mean[b], rstd[b] = mu, rs
    return y, mean, rstd


def emu_instnorm_bwd(x, y, dy, gamma, keep, lens, mean, rstd, lanes):
    L, B, C = x.shape
    order = "lanes%d" % lanes
    dx, dgamma, dbeta = torch.zeros(L, B, C), torch.zeros(C), torch.zeros(C)
    for b in range(B):
        n = min(int(lens[b]), L)
        if n == 0:
            continue
        g = torch.where(y[:n, b] > 0, dy[:n, b], torch.zeros(()))
        if keep is not None:
            g = g * keep[:n, b]
        xh = (x[:n, b] - mean[b]) * rstd[b]
        Sg, Sgx = R.emu_sum(g, order), R.emu_sum(g * xh, order)
        dgamma, dbeta = dgamma + Sgx, dbeta + Sg
        if lanes == 16:
            il = f32(1.0) / n
            dx[:n, b] = gamma * rstd[b] * (g - Sg * il - xh * Sgx * il)
        else:
            dx[:n, b] = gamma * rstd[b] * (g - Sg / n - xh * (Sgx / n))
    return dx, dgamma, dbeta


def worst(name, pairs):
    r = max(R.ratio(got, ref, bound) for got, (ref, bound) in pairs)
    print("%-28s largest |err| / bound = %.4f" % (name, r))
    assert r <= 1.0, (name, r)
    return r


@pytest.mark.parametrize("C,keep,mis,lens,cls", [c for c in G.INORM_CASES if not c[2]])
def test_bounded_instnorm_both_lane_layouts(C, keep, mis, lens, cls):
    x, gamma, beta, k, l32, dy = G.inorm_inputs(C, keep, lens, cls)
    fw = R.instnorm_fwd(x, gamma, beta, k, l32, G.INORM_EPS)
    live = torch.tensor([n > 0 for n in lens])
    y32, m32, r32 = (fw[q][0].float() for q in ("y", "mean", "rstd"))
    bw = R.instnorm_bwd(x, y32, dy, gamma, k, l32, m32, r32)
    for lanes in (4, 16):
        y, mean, rstd = emu_instnorm_fwd(x, gamma, beta, k, l32, G.INORM_EPS, lanes)
        worst("instnorm fwd, %d lanes" % lanes, [(y, fw["y"]), (mean[live], tuple(t[live] for t in fw["mean"])),
                                                 (rstd[live], tuple(t[live] for t in fw["rstd"]))])
        dx, dgamma, dbeta = emu_instnorm_bwd(x, y32, dy, gamma, k, l32, m32, r32, lanes)
        worst("instnorm bwd, %d lanes" % lanes, [(dx, bw["dx"]), (dgamma, bw["dgamma"]), (dbeta, bw["dbeta"])])


@pytest.mark.parametrize("n_rows,M,ext,with_dx", G.AFFINE_CASES[:3] + [G.AFFINE_CASES[-1]])
def test_bounded_coupling(n_rows, M, ext, with_dx):
    out, x, dz, dls = G.affine_inputs(n_rows, M)
    ls, b = out[:, :M], out[:, M:]
    s = torch.exp(ls)
    bw = R.affine_bwd(out, x, dz, dls if ext else None)
    t = dz * x * s
    worst("coupling fwd / bwd / inv", [(s * x + b, R.affine_fwd(out, x)), (torch.cat([t + dls if ext else t, dz], -1), bw["dout"]),
                                       (dz * s, bw["dx"]), ((dz - b) / s, R.affine_inv(out, dz))])


def emu_bce_terms(gate, target, lens):
    T, B = gate.shape
    m = R.frame_mask(lens, T)
    y = target.t()
    return (gate.clamp(min=0) - gate * y + torch.log1p(torch.exp(-gate.abs()))) * m, m, y


@pytest.mark.parametrize("T,B,lens", G.BCE_CASES + [G.PASS2_BCE + (None,)])
def test_bounded_gate_bce(T, B, lens):
    lens = G.full_lens(T, B, 7) if lens is None else torch.tensor(lens, dtype=torch.int32)
    gate, target = G.bce_inputs(T, B, "bounded")
    terms, m, y = emu_bce_terms(gate, target, lens)
    rb = R.gate_bce_fwd(gate, target, lens)
    worst("gate BCE fwd", [(got, rb) for tag, got in flat_orders(terms)])
    if T * B > G.THREADS_BCE:                                        # the launch's own shape under the bound that states its depth
        rd = R.gate_bce_fwd(gate, target, lens, depth=G.bce_depth(T * B, G.THREADS_BCE))
        worst("gate BCE fwd, grid-stride depth", [(R.emu_flat_sum(terms, threads=G.THREADS_BCE, split=s), rd) for s in R.SPLITS])
    sc = f32(0.37) * f32(-1.7)
    worst("gate BCE bwd", [(sc * (1.0 / (1.0 + torch.exp(-gate)) - y) * m, R.gate_bce_bwd(gate, target, lens, float(f32(0.37)), float(f32(-1.7))))])


@pytest.mark.parametrize("T,B,M,n_ls,with_gate,with_dls,lens", G.LOSS_CASES)
def test_bounded_fused_loss(T, B, M, n_ls, with_gate, with_dls, lens):
    lens = torch.tensor(lens, dtype=torch.int32)
    z, lsbuf, gate, target = G.loss_inputs(T, B, M, n_ls, "bounded")
    views = [b[..., :M] for b in lsbuf]
    fw = R.flowtron_loss_fwd(z, views, gate if with_gate else None, target, lens, G.LOSS_SIGMA)
    m = R.frame_mask(lens, T)[:, :, None]
    sl = torch.zeros(T, B, M)
    for v in views:
        sl = sl + v * m
    n = R.emu_sum(lens.clamp(0, T).float(), "seq")
    nm = n * M
    ts2 = f32(2.0) * f32(G.LOSS_SIGMA) * f32(G.LOSS_SIGMA)
    bt = emu_bce_terms(gate, target, lens)[0]
    pairs = []
    for (_, a0), (_, a1), (_, a2) in zip(flat_orders((z * z * m).reshape(T * B, M)), flat_orders(sl.reshape(T * B, M)), flat_orders(bt)):
        pairs += [(a0, fw["acc0"]), (a1, fw["acc1"]), ((a0 / ts2 - a1) / nm, fw["nll"])]
        if with_gate:
            pairs += [(a2, fw["acc2"]), (a2 / n, fw["gate"])]
    pairs += [(1.0 / nm, fw["acc4"]), (1.0 / n, fw["acc5"]), (n, fw["acc6"])]
    worst("fused loss fwd", pairs)
    inv_nm, inv_n = fw["acc4"][0], fw["acc5"][0]
    inv_nm, inv_n = f32(float(inv_nm)), f32(float(inv_n))
    bw = R.flowtron_loss_bwd(z, gate, target, lens, G.LOSS_SIGMA, float(inv_nm), float(inv_n), float(f32(1.3)), float(f32(-0.6)))
    sc = f32(1.3) * inv_nm
    is2 = f32(1.0) / (f32(G.LOSS_SIGMA) * f32(G.LOSS_SIGMA))
    y = target.t()
    worst("fused loss bwd", [((sc * is2) * z * m, bw["dz"]), ((-sc).expand(T, B, M) * m, bw["dls"]),
                             ((f32(-0.6) * inv_n) * (1.0 / (1.0 + torch.exp(-gate)) - y) * m[:, :, 0], bw["dgate"])])


@pytest.mark.parametrize("act", (R.ACT_NONE, R.ACT_TANH, R.ACT_RELU, R.ACT_SIGMOID))
def test_bounded_act_bwd(act):
    y, dy = G.act_inputs(G.ACT_N, act)
    got = {R.ACT_NONE: dy, R.ACT_TANH: dy * (1 - y * y), R.ACT_RELU: torch.where(y > 0, dy, torch.zeros(())), R.ACT_SIGMOID: dy * y * (1 - y)}[act]
    worst("act_bwd %d" % act, [(got, R.act_bwd(y, dy, act))])


@pytest.mark.parametrize("rectified,clipped,wd", ((1, True, True), (0, False, False), (1, False, False)))
def test_bounded_radam(rectified, clipped, wd):
    n = G.RADAM_SMALL
    p, g, m, v = G.radam_inputs(n)
    hp = dict(G.RADAM_HP, weight_decay=G.RADAM_HP["weight_decay"] if wd else 0.0, rectified=rectified)
    gsq = float((g.double() ** 2).sum().float()) * (1.0 if clipped else 1e-6)
    ref = R.radam_step(p, g, m, v, gnorm_sq=gsq, **hp)
    cs = torch.minimum(f32(1.0), f32(hp["clip"]) / (torch.sqrt(f32(gsq)) + f32(1e-6)))
    assert (float(cs) < 1.0) == clipped
    gi = g * cs
    vi = f32(hp["beta2"]) * v + f32(1.0 - hp["beta2"]) * (gi * gi)
    mi = f32(hp["beta1"]) * m + f32(1.0 - hp["beta1"]) * gi
    pi = p - f32(hp["weight_decay"] * hp["lr"]) * p if wd else p
    q = mi / (torch.sqrt(vi) + f32(hp["eps"])) if rectified else mi
    pn = pi - f32(hp["step_size"]) * q
    worst("RAdam step", [(pn, ref["p"]), (mi, ref["m"]), (vi, ref["v"])])


def test_eltwise_reference_is_the_one_fp32_operation():
    for n in (G.ELT_N, G.PASS2_FLAT):
        a, b = R.normal((n,), 1), R.normal((n,), 2)
        assert R.eltwise_inputs_ok(a, b)
        assert torch.equal(R.eltwise(a, b, 0)[0].float(), a + b) and torch.equal(R.eltwise(a, b, 1)[0].float(), a * b)
    assert not R.eltwise_inputs_ok(torch.tensor([1.0]), torch.tensor([2.0 ** -40]))


def test_beta_binomial_reference_rows_are_distributions():
    il, ol = G.prior_lens(3, 17, 9)
    ref, bound = R.beta_binomial_prior(il, ol, 17, 9, 0.05)
    s = ref.sum(-1)
    for b in range(3):
        assert float((s[b, :int(ol[b])] - 1).abs().max()) < 1e-12 and float(s[b, int(ol[b]):].abs().sum()) == 0.0
        assert float(ref[b, :, int(il[b]):].abs().sum()) == 0.0
    assert float((bound[ref > 0] / ref[ref > 0]).max()) < 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------ mutations
def off(mref, rb):
    """how far a wrong reference is from the right one, in bounds"""
    return R.ratio(mref, rb[0], rb[1])


def test_every_wrong_reference_is_caught_at_a_gpu_case():
    seen = {}

    def sharp(mut, dist, exact=False):
        print("%-18s %s" % (mut, "unequal (exact class)" if exact else "%.1f bounds away" % dist))
        assert dist >= R.SHARP, (mut, dist)
        seen[mut] = True

    # instance norm: C 68 on the float4 pair, C 67 on the scalar pair, both with keep (GPU cases of INORM_CASES)
    for C, mut_list in ((68, ("stat_div_L", "var_unbiased", "no_eps", "lane_tail16", "last_quad")), (67, ("lane_tail4",))):
        assert (C, True, False, G.INORM_LENS, "bounded") in G.INORM_CASES
        x, gamma, beta, k, l32, dy = G.inorm_inputs(C, True, G.INORM_LENS, "bounded")
        fw = R.instnorm_fwd(x, gamma, beta, k, l32, G.INORM_EPS)
        for mut in mut_list:
            sharp(mut, off(R.instnorm_fwd(x, gamma, beta, k, l32, G.INORM_EPS, mut=mut)["y"][0], fw["y"]))
        y32, m32, r32 = (fw[q][0].float() for q in ("y", "mean", "rstd"))
        bw = R.instnorm_bwd(x, y32, dy, gamma, k, l32, m32, r32)
        for mut in ("keep_ignored_bwd",) + tuple(m for m in mut_list if m.startswith("lane_tail")):
            mb = R.instnorm_bwd(x, y32, dy, gamma, k, l32, m32, r32, mut=mut)
            sharp(mut, min(off(mb[q][0], bw[q]) for q in ("dx", "dgamma", "dbeta")))
    # masked sums: the strided small case, both classes; the second pass at PASS2_SUMS (exact class)
    T, B, M, ld, lens = G.MSUM_CASES[0]
    l32 = torch.tensor(lens, dtype=torch.int32)
    for cls in ("bounded", "exact"):
        buf = G.msum_inputs(T, B, M, ld, cls)
        for square in (0, 1):
            rb = R.masked_sum(buf, M, l32, square, T, B)
            for mut in ("mask_le", "row_stride"):
                mref = R.masked_sum(buf, M, l32, square, T, B, mut=mut)[0]
                if cls == "exact":
                    assert float(mref) != float(rb[0]), (mut, square)
                elif square:
                    sharp(mut, off(mref, rb))
    T, B, M = G.PASS2_SUMS
    buf, l32 = G.msum_inputs(T, B, M, 2 * M, "exact"), G.full_lens(T, B, 5)
    for square in (0, 1):
        assert float(R.masked_sum(buf, M, l32, square, T, B, mut="pass2", threads=G.THREADS_SUMS)[0]) != float(R.masked_sum(buf, M, l32, square, T, B)[0])
    z, lsbuf, gate, target = G.loss_inputs(T, B, M, 2, "exact")
    views = [b[..., :M] for b in lsbuf]
    l32 = G.full_lens(T, B, 8)
    fw, mw = R.flowtron_loss_fwd(z, views, None, None, l32, G.LOSS_SIGMA), R.flowtron_loss_fwd(z, views, None, None, l32, G.LOSS_SIGMA, mut="pass2", threads=G.THREADS_SUMS)
    assert float(fw["acc0"][0]) != float(mw["acc0"][0]) and float(fw["acc1"][0]) != float(mw["acc1"][0])
    # pass 2 of the elementwise kernels, the BCE sum, the embedding gradient and the optimizer
    n_rows, M = G.PASS2_AFFINE
    out, x, dz, dls = G.affine_inputs(n_rows, M)
    sharp("pass2", off(R.affine_fwd(out, x, mut="pass2", threads=G.THREADS_DEFAULT)[0], R.affine_fwd(out, x)))
    T, B = G.PASS2_BCE
    gate, target = G.bce_inputs(T, B, "bounded")
    l32 = G.full_lens(T, B, 7)
    dep = G.bce_depth(T * B, G.THREADS_BCE)
    sharp("pass2", off(R.gate_bce_fwd(gate, target, l32, mut="pass2", threads=G.THREADS_BCE)[0], R.gate_bce_fwd(gate, target, l32, depth=dep)))
    n, dim, vocab = G.PASS2_EMB
    ids, dob = torch.randint(0, vocab, (n,), generator=R.gen(3)), R.ints((n, dim), 5)
    assert not torch.equal(R.embedding_bwd(ids, dob, vocab, mut="pass2", threads=G.THREADS_DEFAULT)[0], R.embedding_bwd(ids, dob, vocab)[0])
    p, g, m, v = G.radam_inputs(G.PASS2_FLAT)
    hp = dict(G.RADAM_HP, rectified=1)
    ref, mref = R.radam_step(p, g, m, v, gnorm_sq=1e-8, **hp), R.radam_step(p, g, m, v, gnorm_sq=1e-8, mut="pass2", threads=G.THREADS_RADAM, **hp)
    sharp("pass2", min(off(mref[q][0], ref[q]) for q in ("p", "m", "v")))
    # gate target layout, mask_le on the BCE (small cases, T != B)
    T, B, lens = G.BCE_CASES[0]
    gate, target = G.bce_inputs(T, B, "bounded")
    l32 = torch.tensor(lens, dtype=torch.int32)
    sharp("target_TB", off(R.gate_bce_fwd(gate, target, l32, mut="target_TB")[0], R.gate_bce_fwd(gate, target, l32)))
    sharp("target_TB", off(R.gate_bce_bwd(gate, target, l32, 0.37, -1.7, mut="target_TB")[0], R.gate_bce_bwd(gate, target, l32, 0.37, -1.7)))
    sharp("mask_le", off(R.gate_bce_bwd(gate, target, l32, 0.37, -1.7, mut="mask_le")[0], R.gate_bce_bwd(gate, target, l32, 0.37, -1.7)))
    # im2col window, coupling halves
    Ln, B, C, KW, lens = G.IM2COL_CASES[1]
    x, l32 = G.conv_x(Ln, B, C, lens)
    assert KW == 3 and not torch.equal(R.im2col(x, l32, KW, mut="im2col_shift")[0], R.im2col(x, l32, KW)[0])
    seen["im2col_shift"] = True
    n_rows, M, ext, with_dx = G.AFFINE_CASES[3]
    out, x, dz, dls = G.affine_inputs(n_rows, M)
    assert M == 3
    sharp("swap_halves", off(R.affine_fwd(out, x, mut="swap_halves")[0], R.affine_fwd(out, x)))
    # fused loss: 1 / (n M) and a skipped log_s pointer (n_ls 8, bounded and exact)
    T, B, M, n_ls, with_gate, with_dls, lens = G.LOSS_CASES[2]
    l32 = torch.tensor(lens, dtype=torch.int32)
    for cls in ("bounded", "exact"):
        z, lsbuf, gate, target = G.loss_inputs(T, B, M, n_ls, cls)
        views = [b[..., :M] for b in lsbuf]
        fw = R.flowtron_loss_fwd(z, views, gate, target, l32, G.LOSS_SIGMA)
        a = R.flowtron_loss_fwd(z, views, gate, target, l32, G.LOSS_SIGMA, mut="inv_nm_as_inv_n")
        s = R.flowtron_loss_fwd(z, views, gate, target, l32, G.LOSS_SIGMA, mut="skip_ls")
        if cls == "bounded":
            sharp("inv_nm_as_inv_n", off(a["acc4"][0], fw["acc4"]))
            sharp("skip_ls", off(s["acc1"][0], fw["acc1"]))
        else:
            assert float(s["acc1"][0]) != float(fw["acc1"][0])
    # the tail chunk of the runs form: 33 and 65 rows per sequence
    hit = 0
    for n, dim, stride, kind in G.RUNS_CASES:
        ids, dob = G.runs_ids(n, stride, kind, 7), R.ints((n, dim), 6)
        same = torch.equal(R.embedding_bwd(ids, dob, 7, stride=stride, mut="runs_tail")[0], R.embedding_bwd(ids, dob, 7, stride=stride)[0])
        per = -(-n // stride)
        assert same == (per % 32 == 0), (n, stride)
        hit += not same
    assert hit >= 8
    seen["runs_tail"] = True
    assert set(seen) == set(R.MUTATIONS), set(R.MUTATIONS) - set(seen)


# ------------------------------------------------------------------------------------------------------------ index restatements by hand
def test_reverse_by_hand():
    x = torch.arange(5.0).reshape(5, 1, 1).repeat(1, 3, 1)                            # T 5, B 3: value = t
    y = R.reverse_by_length(x, torch.tensor([5, 2, 0], dtype=torch.int32), 1)[0]
    assert y[:, 0, 0].tolist() == [4, 3, 2, 1, 0]
    assert y[:, 1, 0].tolist() == [1, 0, 4, 3, 2]                                     # t >= len: x[T - 1 + len - t] = x[6 - t]
    assert y[:, 2, 0].tolist() == [4, 3, 2, 1, 0]
    yb = R.reverse_by_length(x.transpose(0, 1).contiguous(), torch.tensor([5, 2, 0], dtype=torch.int32), 0)[0]
    assert torch.equal(yb, y.transpose(0, 1))


def test_im2col_window_and_its_adjoint_by_hand():
    x = torch.tensor([1.0, 2.0, 3.0, 0.0]).reshape(4, 1, 1)                           # L 4, len 3
    col = R.im2col(x, torch.tensor([3], dtype=torch.int32), 3)[0]
    assert col[:, 0].tolist() == [[0, 1, 2], [1, 2, 3], [2, 3, 0], [3, 0, 0]]         # row l = x[l - 1], x[l], x[l + 1], 0 outside [0, 3)
    x2 = torch.tensor([[1.0, 10.0], [2.0, 20.0]]).reshape(2, 1, 2)                    # C 2: column c * KW + k
    assert R.im2col(x2, torch.tensor([2], dtype=torch.int32), 3)[0][0, 0].tolist() == [0, 1, 2, 0, 10, 20]
    dcol = torch.arange(12.0).reshape(4, 1, 3)
    dx = R.col2im(dcol, torch.tensor([3], dtype=torch.int32), 1, 3)[0]
    assert dx[:, 0, 0].tolist() == [1 + 3, 2 + 4 + 6, 5 + 7 + 9, 0]                   # dx[l] = dcol[l + 1][0] + dcol[l][1] + dcol[l - 1][2]
    g = R.normal((4, 1, 3), 3).double()
    xr = R.normal((4, 1, 1), 4).double() * torch.tensor([1.0, 1, 1, 0]).reshape(4, 1, 1)
    lens = torch.tensor([3], dtype=torch.int32)
    assert abs(float((R.im2col(xr, lens, 3)[0] * g).sum() - (xr * R.col2im(g, lens, 1, 3)[0]).sum())) < 1e-12      # <im2col x, g> = <x, col2im g>


def test_pad_fill_by_hand():
    y = torch.arange(8.0).reshape(4, 2, 1).reshape(8, 1)                              # T 4, B 2: row t * 2 + b
    lens = torch.tensor([1, 3], dtype=torch.int32)
    assert R.pad_rows_fill(y, lens, 4, 2, 0)[0][:, 0].tolist() == [0, 1, 2, 3, 0, 5, 0, 7]      # b 0: rows t > 1 zeroed; b 1: none (t > 3)
    assert R.pad_rows_fill(y, lens, 4, 2, 1)[0][:, 0].tolist() == [0, 1, 2, 3, 2, 5, 2, 7]      # copies of row (1, 0)


def test_runs_chunking_and_embedding_by_hand():
    n, stride = 70, 2                                                                 # 35 rows per sequence: one full chunk of 32, a tail of 3
    ids = torch.zeros(n, dtype=torch.long)
    dout = torch.ones(n, 1)
    assert float(R.embedding_bwd(ids, dout, 1, stride=stride)[0]) == 70
    assert float(R.embedding_bwd(ids, dout, 1, stride=stride, mut="runs_tail")[0]) == 64
    ids = torch.tensor([2, 0, 2])
    ref = R.embedding_bwd(ids, torch.tensor([[1.0], [5.0], [7.0]]), 3)[0]
    assert ref[:, 0].tolist() == [5, 0, 8]
    assert R.embedding_fwd(ids, torch.tensor([[1.0], [2.0], [3.0]]))[0][:, 0].tolist() == [3, 1, 3]
    m = R.first_pass((3, 4), 10, "cpu")
    assert int(m.sum()) == 10 and not bool(m[2, 2]) and bool(m[2, 1])
