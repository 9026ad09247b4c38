"""tests/cumm_ref64.py checked without a GPU: with the rounding switched off the replay IS the reference's float64 loop and its autograd
gradients (this pins the hand-written adjoint, the halo and the carry); the propagated bounds hold for fp32 emulations of a frame
in several summation orders and splits; and every listed wrong reference is at least SHARP bounds away from the right one on at
least one output, at shapes tests/test_gpu_cumm_f64.py also runs -- which is at the same time the condition on the inputs: the bound
propagated to the LAST backward frame stays 10 x below the smallest mutation's effect."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cumm_ref64 as R

F64 = torch.float64


def make_inputs(T, L, lens, E=640, A=640, f32=True, **kw):
    d, up = R.make_inputs(T, L, lens, E=E, A=A, **kw)
    if not f32:                       # the unrounded mode wants nothing of fp32: perturb every value below its fp32 ulp
        gen = torch.Generator().manual_seed(5)
        d = {k: t * (1 + 1e-9 * torch.randn(t.shape, generator=gen, dtype=F64)) for k, t in d.items()}
        up = {k: t * (1 + 1e-9 * torch.randn(t.shape, generator=gen, dtype=F64)) for k, t in up.items()}
    return d, up


def float64_loop(d, lens, temp):
    """flowtron.py:697-723 + :129-152 + :544-592 in float64 torch with autograd (the loop of tests/test_gpu_ops.py::_cumm_reference,
    restated; it also hands out the running sum and the tanh the kernels save)"""
    T, B, A = d["Q"].shape
    L = d["text"].shape[0]
    cumm, prev = d["Q"].new_zeros(B, 1, L), d["Q"].new_zeros(B, 1, L)
    mask = torch.arange(L)[None, :] >= torch.tensor(lens)[:, None]
    ctxs, attns, lps, cumms, ts = [], [], [], [], []
    for i in range(T):
        cumms.append(cumm[:, 0])
        x = torch.cat([cumm, prev], 1)
        h = torch.relu(F.conv1d(x, d["w1"], d["b1"], padding=2))
        c = torch.sigmoid(F.conv1d(h, d["w2"], d["b2"], padding=1)).permute(2, 0, 1)
        t = torch.tanh(d["Q"][i][None] + (d["text"] * c) @ d["wk"].t())
        ts.append(t)
        e = (t @ d["v"] / temp).t().masked_fill(mask, -float("inf"))
        p = torch.softmax(e, 1)
        ctxs.append(torch.einsum("bl,lba->ba", p, d["V"]))
        attns.append(p)
        lps.append(torch.log(p + R.EPS_LP))
        prev = p[:, None, :]
        cumm = cumm + prev
    return torch.stack(ctxs, 0), torch.stack(attns, 1), torch.stack(lps, 1), torch.stack(cumms, 0), torch.stack(ts, 0)


def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("T,L,lens", [(3, 33, [33, 27, 1]), (4, 9, [9, 3])])
@pytest.mark.parametrize("ups", ["all", "dctx", "last", "first"])
def test_unrounded_replay_is_the_float64_loop_and_its_autograd(T, L, lens, ups):
    d, up = make_inputs(T, L, lens, E=64, A=96, f32=False)
    temp = 0.875
    if ups == "last":
        up["dctx"][:-1] = 0
    if ups == "first":
        up["dctx"][1:] = 0
    leaves = {k: t.clone().requires_grad_(True) for k, t in d.items()}
    ctx, attn, lp, cumm, ts = float64_loop(leaves, lens, temp)
    loss = (ctx * up["dctx"]).sum()
    if ups == "all":
        loss = loss + (attn * up["dattn"]).sum() + (lp * up["dlp"]).sum()
    loss.backward()
    P = R.Params(**d, in_lens=lens, temp=temp)
    st = R.State(attn.detach(), cumm.detach(), ts.detach(), P)
    vl = P.valid.t()[:, :, None]
    for i in range(T):
        f = R.frame_fwd(P, st, i, None)
        assert rel(f["saved"].v * vl, ts[i].detach() * vl) < 1e-12
        assert rel(f["attn"].v, attn[:, i].detach()) < 1e-12
        assert rel(f["logprob"].v, lp[:, i].detach()) < 1e-12
    assert rel(R.ctx_ref(P, st, None).v, ctx.detach()) < 1e-12
    g = R.replay_bwd(P, st, up["dctx"], up["dattn"] if ups == "all" else None, up["dlp"] if ups == "all" else None, None)
    for name, key in zip(R.OUT_BWD, ("Q", "V", "text", "wk", "v", "w1", "b1", "w2", "b2")):
        assert rel(g[name].v, leaves[key].grad) < 1e-12, (name, rel(g[name].v, leaves[key].grad))


# ------------------------------------------------------------------------------------------------------------------ sharpness
# cold: a low temperature, so that some attention weights fall below the 1e-8 of logprob (its gradient factor shows only there)
# tight is T = 2: the first backward frame starts without a carry and the second holds the once-propagated bound (~100 x wider); by
# T = 3 a one-row mutation such as halo_zero is no longer 10 bounds away
CASES = {"tight": (2, 33, [33, 27, 1], 0.9, 0.3), "chunk": (9, 33, [33, 27, 1], 0.9, 1e-3), "cold": (2, 33, [33, 27, 1], 0.3, 0.3)}
_cache = {}


def case(name, fmt):
    if (name, fmt) not in _cache:
        T, L, lens, temp, w1s = CASES[name]
        d, up = make_inputs(T, L, lens, w1_scale=w1s)
        P = R.Params(**d, in_lens=lens, temp=temp)
        st = R.simulate_fwd(P, fmt)
        chunk = 4 if name == "chunk" else None
        fw = [R.frame_fwd(P, st, i, fmt) for i in range(T)]
        bw = R.replay_bwd(P, st, up["dctx"], up["dattn"], up["dlp"], fmt, chunk=chunk)
        _cache[(name, fmt)] = (P, st, up, chunk, fw, bw)
    return _cache[(name, fmt)]


def away(wrong, right, mask=None):
    """how many bounds the wrong reference lies from the right one, at its worst element"""
    err, bound = (wrong.v - right.v).abs(), right.err()
    if mask is not None:
        err, bound = err[mask.expand_as(err)], bound[mask.expand_as(err)]
    return float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("mut", R.MUT_FWD)
def test_wrong_forward_references_are_ten_bounds_away(mut, fmt):
    P, st, up, chunk, fw, bw = case("tight", fmt)
    vl = P.valid.t()[:, :, None]
    worst = {}
    for i in range(1, P.T):
        f = R.frame_fwd(P, st, i, fmt, mut)
        for k, m in (("saved", vl), ("attn", None), ("logprob", None)):
            worst[k] = max(worst.get(k, 0.0), away(f[k], fw[i][k], m))
    print("\n[cumm sharpness fwd fmt %d] %s: %s" % (fmt, mut, {k: "%.3g" % x for k, x in worst.items()}))
    assert max(worst.values()) >= R.SHARP, worst


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("mut", R.MUT_BWD)
def test_wrong_backward_references_are_ten_bounds_away(mut, fmt):
    P, st, up, chunk, fw, bw = case({"top_chunk": "chunk", "no_eps": "cold"}.get(mut, "tight"), fmt)
    g = R.replay_bwd(P, st, up["dctx"], up["dattn"], up["dlp"], fmt, chunk=chunk, mut=mut)
    worst = {k: away(g[k], bw[k]) for k in R.OUT_BWD}
    print("\n[cumm sharpness bwd fmt %d] %s: %s" % (fmt, mut, {k: "%.3g" % x for k, x in worst.items()}))
    assert max(worst.values()) >= R.SHARP, worst
    if mut == "top_chunk":
        assert min(worst["dw_key"], worst["dw2"]) >= R.SHARP, worst
    if mut == "db2_one":
        assert worst["db2"] >= R.SHARP, worst


@pytest.mark.parametrize("fmt", [1, 2])
def test_bound_at_the_last_backward_frame_is_small_against_the_carry(fmt):
    """condition on the inputs: after the whole scan (frame 0 is the LAST backward frame) the never-reset bound of the (dprev, dcumm)
    carry is still 10 x below what the smallest carry mutation (the carry of frame i+1 dropped) changes in it"""
    for name in ("tight", "cold"):                  # (chunk: the carry is scaled away on purpose; top_chunk / db2_one are its mutations)
        P, st, up, chunk, fw, bw = case(name, fmt)
        g = R.replay_bwd(P, st, up["dctx"], up["dattn"], up["dlp"], fmt, chunk=chunk, mut="no_carry")
        for k in (0, 1):
            assert away(g["carry"][k], bw["carry"][k], P.valid) >= R.SHARP, (name, k)
            ratio = float((bw["carry"][k].err() / bw["carry"][k].v.abs().clamp_min(1e-300))[P.valid].median())
            assert ratio < 0.1, (name, k, ratio)


# ------------------------------------------------------------------------------------------------------------------ the bounds hold
def sum32(terms, order, parts, rng):
    """fp32 sum over the last axis: the terms in `order` (fwd / rev / shuffle), cut into `parts` runs that are summed one element after
    the other (numpy's accumulate is sequential) and then combined one after the other"""
    K = terms.shape[-1]
    idx = {"fwd": np.arange(K), "rev": np.arange(K)[::-1], "shuffle": rng.permutation(K)}[order]
    t = terms[..., idx].astype(np.float32)
    cuts = np.linspace(0, K, min(parts, K) + 1).astype(int)
    partial = [np.cumsum(t[..., a:b], axis=-1, dtype=np.float32)[..., -1] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    return np.cumsum(np.stack(partial, -1), axis=-1, dtype=np.float32)[..., -1]


def mfma32(a, b, order, parts, rng):
    """a [M, K] . b [N, K]^T the way cumm_ref64 assumes the matrix cores add: products of 16-bit operands are exact in fp32; the 32
    products of one instruction are added in some order with fp32 roundings (sum32), the instructions chain on one accumulator"""
    M, K = a.shape
    acc = np.zeros((M, b.shape[0]), np.float32)
    for k0 in range(0, K, 32):
        prod = a[:, None, k0:k0 + 32].astype(np.float32) * b[None, :, k0:k0 + 32].astype(np.float32)
        acc = (acc + sum32(prod, order, parts, rng)).astype(np.float32)
    return acc


def fn32(fn, x):
    """a correctly rounded fp32 function (float64 evaluation, one rounding)"""
    return fn(x.astype(np.float64)).astype(np.float32)


def emulate_frame(P, st, i, fmt, order, parts, rng):
    """one forward frame of the fused kernel in numpy.float32, from the saved state, with the kernel's roundings"""
    f = np.float32
    r16 = lambda x: R.rnd(torch.from_numpy(np.ascontiguousarray(x)).double(), fmt).numpy().astype(f)
    n = lambda t: t.numpy().astype(f)
    B, L, E, A = P.B, P.L, P.E, P.A
    prev = st.attn[:, i - 1] if i > 0 else torch.zeros_like(st.cumm[0])
    x = torch.stack([st.cumm[i], prev], 1)
    xu = n(F.pad(x, (2, 2)).unfold(2, 5, 1))                                                     # [B, 2, L, 5]
    prod = (n(P.w1)[None, :, :, None, :] * xu[:, None]).astype(f)                                 # [B, NF, 2, L, 5]
    terms = np.concatenate([prod.transpose(0, 1, 3, 2, 4).reshape(B, 32, L, 10), np.broadcast_to(n(P.b1)[None, :, None, None], (B, 32, L, 1))], -1)
    h1 = np.maximum(sum32(terms, order, parts, rng), f(0))                                        # [B, NF, L]
    col2 = torch.from_numpy(r16(h1)).double()
    cu = n(F.pad(col2, (1, 1)).unfold(2, 3, 1).permute(2, 0, 1, 3).reshape(L * B, 96))           # row l * B + b, tap c * 3 + k
    pre2 = (mfma32(cu, r16(n(P.w2).reshape(E, 96)), order, parts, rng) + n(P.b2)[None]).astype(f)
    cond = fn32(lambda z: 1 / (1 + np.exp(-z)), pre2)
    km = r16((n(P.text).reshape(L * B, E) * cond).astype(f))
    K = mfma32(km, r16(n(P.wk)), order, parts, rng)
    t = fn32(np.tanh, (n(P.Q[i])[None].repeat(L, 0).reshape(L * B, A) + K).astype(f)).reshape(L, B, A)
    # downstream of the saved tanh (the state's): scores as 32 runs of 20 products, then a tree; softmax; logprob of the state's attn
    ts = n(st.kproj[i])
    pv = (ts * n(P.v)).astype(f).reshape(L, B, 32, 20)
    part = sum32(pv, order, 1, rng)
    while part.shape[-1] > 1:
        part = (part[..., 0::2] + part[..., 1::2]).astype(f)
    e = (part[..., 0] * f(1.0 / f(P.temp))).astype(f).T                                           # [B, L]
    attn = np.zeros((B, L), f)
    for b in range(B):
        ln = P.lens[b]
        z = fn32(np.exp, (e[b, :ln] - e[b, :ln].max()).astype(f))
        attn[b, :ln] = (z / sum32(z[None], order, parts, rng)[0]).astype(f)
    lp = fn32(np.log, (n(st.attn[:, i]) + f(1e-8)).astype(f))
    return t, attn, lp


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("parts", [1, 3, 8])
@pytest.mark.parametrize("order", ["fwd", "rev", "shuffle"])
def test_bounds_hold_for_fp32_emulations_of_a_frame(order, parts, fmt):
    """numpy.float32 restatements of a forward frame -- forward, reverse and shuffled summation order; one, three and many partial
    sums; both 16-bit formats -- stay within the replay's bounds"""
    T, L, lens = 2, 7, [7, 4]
    for cls in ("aligned", "signed"):
        d, up = make_inputs(T, L, lens, cls=cls)
        P = R.Params(**d, in_lens=lens, temp=0.9)
        st = R.simulate_fwd(P, fmt)
        rng = np.random.default_rng(3)
        t, attn, lp = emulate_frame(P, st, 1, fmt, order, parts, rng)
        fr = R.frame_fwd(P, st, 1, fmt)
        vl = P.valid.t()[:, :, None]
        worst = {}
        for name, got, ref, m in (("tanh", t, fr["saved"], vl), ("attn", attn, fr["attn"], P.valid), ("logprob", lp, fr["logprob"], None)):
            err, bound = (torch.from_numpy(got).double() - ref.v).abs(), ref.err()
            if m is not None:
                err, bound = err[m.expand_as(err)], bound[m.expand_as(err)]
            worst[name] = float((err / bound.clamp_min(1e-300)).max())
        print("\n[cumm bounds fmt %d %s parts %d %s] error / bound: %s" % (fmt, order, parts, cls, {k: "%.3g" % x for k, x in worst.items()}))
        assert max(worst.values()) <= 1.0, worst
        assert float(attn[~P.valid.numpy()].sum()) == 0.0
