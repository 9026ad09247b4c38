"""Float64 restatement of the elementwise, gather, norm, loss and optimizer entry points of include/flowtron_hip.h (csrc/elementwise.hip,
csrc/instnorm.hip), two input classes, a per-element error bound and the wrong references of the sensitivity check (imported by
tests/test_elementwise_ref64_cpu.py and tests/test_gpu_elementwise_f64.py, not collected).  Plain torch on whatever device the inputs
live on; nothing here calls the project's kernels, and every formula is the header's, not a kernel's.

Every restatement returns (reference, bound), float64, element by element (a dict of such pairs where an entry point has several
outputs).  bound 0 = the element must come back EQUAL (copies, masks, padding).

Input class "exact": data are small integers (or multiples of a small power of two), keep in {0, 2}, targets in {0, 1}.  Every
partial sum in any order and any split is then a multiple of the grid and below 2^24 of it (`assert_exact` asserts it from the float64
magnitudes), so fp32 arithmetic rounds nowhere and a correct kernel equals the reference BIT FOR BIT, float atomics included.  This is
the class that carries the long reductions.

Input class "bounded": N(0, 1)-scaled data under |got - ref| <= bound, u = U = 2^-23 (one whole ulp per rounding, so a truncating
implementation passes too):
  * one u per rounding the formula needs (times the magnitude of the value rounded);
  * a sum of n terms in ANY order and any split over lanes, waves, workgroups and atomics: n * u * sum |terms| (every term passes
    through fewer than n additions, each rounding a partial sum no larger than sum |terms|) -- no lane layout is assumed;
  * the instance norm propagates the error of the mean and of the variance through rstd and xhat (instnorm_fwd's comments);
  * device math functions at the OpenCL full-profile limits (OpenCL C specification, "Relative error as ULPs", the limits the ROCm
    device library implements for expf / log1pf / sqrtf / fp32 division without fast-math): EXP_ULP, LOG1P_ULP, SQRT_ULP, DIV_ULP;
  * results that may underflow get the absolute floor FLT_MIN (a flushed subnormal still compares).
These limits are generous on purpose; what keeps the tests from being slack is MUTATIONS: wrong references one line away from the
right one, each of which must lie SHARP bounds away (exact class: be unequal) at a shape the GPU file runs."""
import math

import torch

U = 2.0 ** -23
SHARP = 10.0
F64 = torch.float64
EXP_ULP, LOG1P_ULP, SQRT_ULP, DIV_ULP = 3.0, 2.0, 3.0, 2.5         # OpenCL C full profile: exp <= 3 ulp, log1p <= 2, sqrt <= 3, x / y <= 2.5
FLT_MIN = 2.0 ** -126
FLT_SUBNORMAL = 2.0 ** -149
LGAMMA_ULP64 = 16.0                                                # float64 lgamma, reference's and device's together (no published limit; 16 ulp
#                                                                    of 2^-53 at |lgamma| ~ 1e4 is 2e-11, far below the fp32 rounding it sits beside)
ACT_NONE, ACT_TANH, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3
RUNS_RB = 32                                                       # rows per run chunk of ft_embedding_bwd_runs (mutation runs_tail only)

MUTATIONS = ("stat_div_L", "var_unbiased", "no_eps", "lane_tail16", "lane_tail4", "last_quad", "keep_ignored_bwd", "mask_le",
             "target_TB", "row_stride", "pass2", "im2col_shift", "swap_halves", "inv_nm_as_inv_n", "skip_ls", "runs_tail")


def gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def ints(shape, seed, lim=4):
    """exact class: integers in [-lim, lim] as fp32"""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=gen(seed)).float()


def normal(shape, seed, scale=1.0):
    return torch.randn(tuple(shape), generator=gen(seed)) * scale


def d(t):
    return t.to(F64)


def ratio(got, ref, bound):
    """largest |got - ref| / bound; elements with bound 0 must be equal (ratio inf otherwise); NaN counts as inf"""
    got, ref, bound = (torch.as_tensor(t, dtype=F64).reshape(-1) for t in (got, ref, bound))
    ref, bound = ref.to(got.device), bound.to(got.device)
    e = (got - ref).abs()
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    r = torch.where(bound > 0, e / bound.clamp(min=1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
    return float(r.max()) if r.numel() else 0.0


def assert_exact(abs_total, unit=1.0, *tensors):
    """the condition under which the exact class IS exact: every value is a multiple of `unit` (a power of two) and the largest possible
    total, the sum of ALL magnitudes, is below 2^24 units -- then so is every partial sum in every order, and fp32 holds each exactly"""
    assert math.frexp(unit)[0] == 0.5
    assert float(abs_total) / unit < 2.0 ** 24, (float(abs_total), unit)
    for t in tensors:
        q = d(t) / unit
        assert bool((q == q.round()).all())


def frame_mask(lens, T, mut=None):
    """[T, B] bool: t < lens[b] (the header's "valid"); mutation mask_le: t <= lens[b]"""
    t = torch.arange(T, device=lens.device)[:, None]
    return (t <= lens[None, :]) if mut == "mask_le" else (t < lens[None, :])


def first_pass(shape, threads, device):
    """bool of `shape`: flat index < threads (what the first grid-stride pass of a launch of `threads` threads covers; mutation pass2)"""
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n, device=device) < threads).reshape(shape)


# ------------------------------------------------------------------------------------------------------------ embedding
def embedding_fwd(ids, W):
    """out[r] = W[ids[r]]"""
    ref = d(W)[ids]
    return ref, torch.zeros_like(ref)


def embedding_bwd(ids, dout, vocab, *, stride=None, mut=None, threads=None):
    """dW[ids[r]] += dout[r] from dW = 0 (ft_embedding_bwd and, with `stride`, ft_embedding_bwd_runs: the same sums).  dout [n, dim]."""
    n, dim = dout.shape
    g = d(dout)
    if mut == "pass2":
        g = g * first_pass((n, dim), threads, g.device)
    if mut == "runs_tail":                                         # rows past the last full chunk of RUNS_RB rows of their sequence j = r % stride
        per = -(-n // stride)
        i = torch.arange(n, device=g.device) // stride
        g = g * (i < RUNS_RB * (per // RUNS_RB))[:, None]
    ref = torch.zeros(vocab, dim, dtype=F64, device=g.device).index_add_(0, ids, g)
    mag = torch.zeros(vocab, dim, dtype=F64, device=g.device).index_add_(0, ids, g.abs())
    cnt = torch.zeros(vocab, dtype=F64, device=g.device).index_add_(0, ids, torch.ones(n, dtype=F64, device=g.device))
    return ref, cnt[:, None] * U * mag


# ------------------------------------------------------------------------------------------------------------ im2col / col2im
def im2col(x, lens, KW, mut=None):
    """col[l][b][c * KW + k] = x[l + k - KW / 2][b][c], 0 outside [0, lens[b]).  x [L, B, C]."""
    L, B, C = x.shape
    h = KW // 2 - (1 if mut == "im2col_shift" else 0)
    l = torch.arange(L, device=x.device)
    col = torch.zeros(L, B, C, KW, dtype=F64, device=x.device)
    for k in range(KW):
        ls = l + k - h
        ok = ((ls >= 0) & (ls < L))[:, None] & (ls[:, None] < lens[None, :])
        col[..., k] = torch.where(ok[:, :, None], d(x)[ls.clamp(0, L - 1)], torch.zeros((), dtype=F64, device=x.device))
    col = col.reshape(L, B, C * KW)
    return col, torch.zeros_like(col)


def col2im(dcol, lens, C, KW):
    """the adjoint: dx[l][b][c] = sum_k dcol[l - k + KW / 2][b][c * KW + k] over rows inside [0, L), 0 at l >= lens[b]"""
    L, B, _ = dcol.shape
    g = d(dcol).reshape(L, B, C, KW)
    h = KW // 2
    l = torch.arange(L, device=dcol.device)
    ref = torch.zeros(L, B, C, dtype=F64, device=dcol.device)
    mag = torch.zeros_like(ref)
    for k in range(KW):
        lo = l - k + h
        ok = ((lo >= 0) & (lo < L))[:, None, None]
        v = torch.where(ok, g[lo.clamp(0, L - 1)][..., k], torch.zeros((), dtype=F64, device=dcol.device))
        ref += v
        mag += v.abs()
    m = frame_mask(lens, L)[:, :, None]
    return ref * m, KW * U * mag * m


# ------------------------------------------------------------------------------------------------------------ reverse by length
def reverse_by_length(x, lens, time_major):
    """y[t] = x[len - 1 - t] (t < len), x[T - 1 + len - t] (t >= len); 0 <= len <= T"""
    xt = d(x) if time_major else d(x).transpose(0, 1)
    T, B, _ = xt.shape
    t = torch.arange(T, device=x.device)[:, None]
    ln = lens[None, :].long()
    src = torch.where(t < ln, ln - 1 - t, T - 1 + ln - t)
    y = xt[src, torch.arange(B, device=x.device)[None, :]]
    y = y if time_major else y.transpose(0, 1).contiguous()
    return y, torch.zeros_like(y)


# ------------------------------------------------------------------------------------------------------------ instance norm + ReLU
def _stat_mask(lens, L, mut):
    n = lens.clamp(max=L).long()
    l = torch.arange(L, device=lens.device)[:, None]
    m = l < n[None, :]
    sm = m
    if mut == "lane_tail16":
        sm = m & (l < 16 * (n // 16))
    if mut == "lane_tail4":
        sm = m & (l < 4 * (n // 4))
    return n, m, sm


def instnorm_fwd(x, gamma, beta, keep, lens, eps, mut=None):
    """x [L, B, C]; n_b = min(lens[b], L); mean, biased variance over l < n_b; rstd = 1 / sqrt(var + eps) (eps as the fp32 the ABI passes);
    y = relu((x - mean) rstd gamma + beta) * keep at l < n_b, 0 beyond.  Samples with n_b = 0: y = 0, statistics not defined (returned 0
    with bound inf: not compared).  Returns {"y", "mean", "rstd"} -> (ref, bound)."""
    L, B, C = x.shape
    X = d(x)
    n, m, sm = _stat_mask(lens, L, mut)
    m3, sm3 = m[:, :, None], sm[:, :, None]
    nn = n.clamp(min=1).to(F64)[:, None]                           # [B, 1]
    div = torch.full_like(nn, float(L)) if mut == "stat_div_L" else nn
    e32 = float(torch.tensor(eps, dtype=torch.float32))
    S = (X * sm3).sum(0)
    absS = (X.abs() * m3).sum(0)
    mean = S / div
    # mean: n additions in any order, then S / n or S * (1 / n): a division and at most one more rounding
    dm = U * absS + (DIV_ULP + 1) * U * mean.abs()               # (n u sum |x|) / n
    dd = (X - mean[None]) * m3
    e = (dm[None] + U * (dd.abs() + dm[None])) * m3               # error of the computed x - mean: the mean's, and the subtraction's rounding
    Q = (dd * dd * sm3).sum(0)
    hi2 = (dd.abs() + e) ** 2
    dQ = (2 * dd.abs() * e + e * e).sum(0) + U * hi2.sum(0) + nn * U * hi2.sum(0)     # squares of perturbed terms, their rounding, n additions
    vdiv = (div - 1).clamp(min=1) if mut == "var_unbiased" else div
    var = Q / vdiv
    dv = dQ / nn + (DIV_ULP + 1) * U * (var + dQ / nn)
    w = var + (0.0 if mut == "no_eps" else e32)
    dw = dv + U * (w + dv)
    rstd = 1.0 / torch.sqrt(w)
    wlo = (w - dw).clamp(min=1e-300)
    dr = rstd * (SQRT_ULP + DIV_ULP) * U + (1.0 / torch.sqrt(wlo) - rstd)            # sqrt and division, and the whole interval of w
    h = dd * rstd[None]
    dh = e * (rstd + dr)[None] + dd.abs() * dr[None] + U * (h.abs() + e * rstd[None])
    G, Be = d(gamma)[None, None, :], d(beta)[None, None, :]
    t = h * G + Be
    dt = G.abs() * dh + U * (h.abs() + dh) * G.abs() + U * ((h.abs() + dh) * G.abs() + Be.abs())
    y = t.clamp(min=0.0)
    dy = dt                                                        # relu: Lipschitz 1
    if keep is not None:
        K = d(keep)
        y = y * K
        dy = K.abs() * dt + U * y.abs()
    y, dy = y * m3, dy * m3
    inf = torch.full_like(mean, float("inf"))
    lb = (n > 0)[:, None]
    out = {"y": (y, dy), "mean": (torch.where(lb, mean, torch.zeros_like(mean)), torch.where(lb, dm, inf)),
           "rstd": (torch.where(lb, rstd, torch.zeros_like(rstd)), torch.where(lb, dr, inf))}
    if mut == "last_quad" and C % 64:                              # the last channel quad of the partial slab never written
        for k in out:
            out[k][0][..., C - 4:] = 0.0
    return out


def instnorm_bwd(x, y, dy, gamma, keep, lens, mean, rstd, mut=None):
    """The derivative of instnorm_fwd with the SAVED y, mean, rstd as inputs (fp32, exact): g = (y > 0 ? dy : 0) * keep, xhat = (x - mean)
    rstd, dbeta[c] = sum_{b, l < n_b} g, dgamma[c] = sum g xhat, dx = gamma rstd (g - Sg_b / n_b - xhat Sgx_b / n_b), 0 at l >= n_b.
    Returns {"dx", "dgamma", "dbeta"} -> (ref, bound)."""
    L, B, C = x.shape
    n, m, sm = _stat_mask(lens, L, mut)
    m3, sm3 = m[:, :, None], sm[:, :, None]
    nn = n.clamp(min=1).to(F64)[:, None]
    live = (n > 0)[:, None]
    Mn = torch.where(live, d(mean), torch.zeros_like(d(mean)))
    Rs = torch.where(live, d(rstd), torch.zeros_like(d(rstd)))
    g = torch.where(d(y) > 0, d(dy), torch.zeros_like(d(dy)))
    dg = torch.zeros_like(g)
    if keep is not None and mut != "keep_ignored_bwd":
        g = g * d(keep)
        dg = U * g.abs()
    g, dg = g * m3, dg * m3
    xh = (d(x) - Mn[None]) * Rs[None] * m3
    dxh = 2 * U * xh.abs()
    gx = g * xh
    dgx = g.abs() * dxh + dg * (xh.abs() + dxh) + U * gx.abs()
    Sg, Sgx = (g * sm3).sum(0), (gx * sm3).sum(0)
    dSg = dg.sum(0) + nn * U * g.abs().sum(0)
    dSgx = dgx.sum(0) + nn * U * (gx.abs() + dgx).sum(0)
    N = float(n.sum().clamp(min=1))
    dbeta, dgamma = Sg.sum(0), Sgx.sum(0)
    b_dbeta = dg.sum((0, 1)) + N * U * g.abs().sum((0, 1))
    b_dgamma = dgx.sum((0, 1)) + N * U * (gx.abs() + dgx).sum((0, 1))
    A, Bq = Sg / nn, Sgx / nn
    dA = dSg / nn + (DIV_ULP + 1) * U * (A.abs() + dSg / nn)
    dB = dSgx / nn + (DIV_ULP + 1) * U * (Bq.abs() + dSgx / nn)
    t3 = xh * Bq[None]
    d3 = dxh * (Bq.abs() + dB)[None] + xh.abs() * dB[None] + U * t3.abs()
    inner = g - A[None] - t3
    dinner = dg + dA[None] + d3 + 2 * U * (g.abs() + A.abs()[None] + t3.abs() + dA[None] + d3)
    gr = (d(gamma)[None, :] * Rs)[None]
    dx = gr * inner * m3
    ddx = (gr.abs() * dinner + 2 * U * gr.abs() * (inner.abs() + dinner)) * m3
    return {"dx": (dx, ddx), "dgamma": (dgamma, b_dgamma), "dbeta": (dbeta, b_dbeta)}


# ------------------------------------------------------------------------------------------------------------ affine coupling
def _halves(out, M, mut):
    o = d(out)
    ls, b = o[..., :M], o[..., M:]
    return (b, ls) if mut == "swap_halves" else (ls, b)


def affine_fwd(out, x, mut=None, threads=None):
    """out [n, 2M] = [log_s | b]; z = exp(log_s) x + b"""
    M = x.shape[-1]
    ls, b = _halves(out, M, mut)
    ex = torch.exp(ls) * d(x)
    z = ex + b
    bound = U * ((EXP_ULP + 1) * ex.abs() + ex.abs() + b.abs())    # exp, the product, the addition
    if mut == "pass2":
        z = z * first_pass(z.shape, threads, z.device)
    return z, bound


def affine_bwd(out, x, dz, dls_ext):
    """dout = [dz x exp(log_s) + dlog_s_ext | dz], dx = dz exp(log_s).  Returns {"dout", "dx"}."""
    M = x.shape[-1]
    ls, _ = _halves(out, M, None)
    s, g = torch.exp(ls), d(dz)
    t = g * d(x) * s
    bt = (EXP_ULP + 2) * U * t.abs()
    dls = t
    if dls_ext is not None:
        dls = t + d(dls_ext)
        bt = bt + U * (t.abs() + d(dls_ext).abs())
    dx = g * s
    return {"dout": (torch.cat([dls, g], -1), torch.cat([bt, torch.zeros_like(g)], -1)), "dx": (dx, (EXP_ULP + 1) * U * dx.abs())}


def affine_inv(out, z):
    """x = (z - b) / exp(log_s)"""
    M = z.shape[-1]
    ls, b = _halves(out, M, None)
    x = (d(z) - b) / torch.exp(ls)
    return x, (1 + DIV_ULP + EXP_ULP + 1) * U * x.abs()              # the subtraction, the division, exp, the result's rounding


# ------------------------------------------------------------------------------------------------------------ masked sums
def masked_sum(buf, M, lens, square, T, B, mut=None, threads=None):
    """buf [T * B, ld] (x = its first M columns, row stride ld); sum over t < lens[b] of x (square = 0) or x^2.  Returns scalars."""
    X = d(buf)[:, :M]
    if mut == "row_stride":                                        # row * M for row * ld
        X = d(buf).reshape(-1)[:T * B * M].reshape(T * B, M)
    m = frame_mask(lens, T, mut).reshape(T * B, 1)
    if mut == "pass2":
        m = m & first_pass((T * B, M), threads, buf.device)
    t = (X * X if square else X) * m
    n = float(m.expand(T * B, M).sum())
    return t.sum(), U * (n + (1 if square else 0)) * t.abs().sum()


def masked_sum_bwd(buf, M, lens, scale, coef, square, T, B):
    """dx = scale * coef * (square ? x : 1) at valid positions, 0 at pads; [T * B, M]"""
    sc = float(scale) * float(coef)
    m = frame_mask(lens, T).reshape(T * B, 1)
    v = (sc * d(buf)[:, :M] if square else torch.full((T * B, M), sc, dtype=F64, device=lens.device)) * m
    return v, (2 if square else 1) * U * v.abs()


# ------------------------------------------------------------------------------------------------------------ gate BCE
def _bce_terms(gate, target, lens, mut):
    T, B = gate.shape
    g = d(gate)
    y = d(target).reshape(-1)[:T * B].reshape(T, B) if mut == "target_TB" else d(target).t()
    m = frame_mask(lens, T, mut)
    return g, y, m


def gate_bce_fwd(gate, target, lens, mut=None, threads=None, depth=None):
    """gate [T, B], target [B, T]; sum over valid frames of max(g, 0) - g y + log1p(exp(-|g|)).  depth: the most additions one term passes
    through, where the caller can state it (a grid-stride launch: passes per thread + the workgroup's tree + one atomic per workgroup);
    None: any order at all (the number of terms)."""
    g, y, m = _bce_terms(gate, target, lens, mut)
    if mut == "pass2":
        m = m & first_pass(g.shape, threads, g.device)
    e = torch.exp(-g.abs())
    lp = torch.log1p(e)
    pos, gy = g.clamp(min=0.0), g * y
    term = (pos - gy + lp) * m
    # exp (propagated through log1p, whose slope is <= 1), log1p, the product, two additions; FLT_MIN: exp(-|g|) may be flushed
    dterm = (U * (EXP_ULP * e + LOG1P_ULP * lp + gy.abs() + 2 * (pos + gy.abs() + lp)) + FLT_MIN) * m
    n = float(m.sum())
    mag = ((pos + gy.abs() + lp) * m).sum()
    return term.sum(), dterm.sum() + (n if depth is None else min(n, depth)) * U * mag


def _sigmoid_err(g):
    """sigmoid as 1 / (1 + exp(-g)): exp, the addition, the division; an exp that overflows gives 0 for a value below FLT_MIN"""
    s = torch.sigmoid(g)
    return s, (EXP_ULP + 1 + DIV_ULP) * U * s + FLT_MIN


def gate_bce_bwd(gate, target, lens, scale, coef, mut=None):
    """dgate = scale * coef * (sigmoid(g) - y) at valid frames, 0 at pads"""
    g, y, m = _bce_terms(gate, target, lens, mut)
    sc = float(scale) * float(coef)
    s, ds = _sigmoid_err(g)
    v = sc * (s - y) * m
    return v, (abs(sc) * (ds + U * (s - y).abs()) + 2 * U * v.abs()) * m


# ------------------------------------------------------------------------------------------------------------ fused loss
def flowtron_loss_fwd(z, ls_list, gate, target, lens, sigma, mut=None, threads=None):
    """z [T, B, M]; ls_list: up to 8 [T, B, M] views; gate [T, B] / target [B, T] or None.  n = sum_b min(max(lens[b], 0), T).
    Returns {"acc0", "acc1", "acc2", "acc4", "acc5", "acc6", "nll", "gate"} -> (ref, bound) scalars."""
    T, B, M = z.shape
    m = frame_mask(lens, T, mut)[:, :, None]
    if mut == "pass2":
        m = m & first_pass((T, B, M), threads, z.device)
    nv = float(m.expand(T, B, M).sum())
    z2 = d(z) ** 2 * m
    a0, b0 = z2.sum(), U * (nv + 1) * z2.sum()
    use = list(ls_list)[1:] if mut == "skip_ls" else list(ls_list)
    a1 = torch.zeros((), dtype=F64, device=z.device)
    mag1 = torch.zeros((), dtype=F64, device=z.device)
    for v in use:
        a1 = a1 + (d(v) * m).sum()
        mag1 = mag1 + (d(v).abs() * m).sum()
    b1 = U * nv * max(len(ls_list), 1) * mag1
    n = float(lens.clamp(min=0, max=T).sum())
    nm = n if mut == "inv_nm_as_inv_n" else n * M
    assert n * M < 2.0 ** 24                                       # n M is formed in fp32: exact
    s32 = float(torch.tensor(sigma, dtype=torch.float32))
    ts2 = 2.0 * s32 * s32
    A = a0 / ts2
    dA = b0 / ts2 + (1 + DIV_ULP) * U * A.abs()                    # 2 sigma^2 rounded once, the division
    num = A - a1
    dnum = dA + b1 + U * (A.abs() + a1.abs() + dA + b1)
    nll = num / (n * M)
    out = {"acc0": (a0, b0), "acc1": (a1, b1), "acc4": (1.0 / nm, DIV_ULP * U / nm), "acc5": (1.0 / n, DIV_ULP * U / n), "acc6": (n, 0.0),
           "nll": (nll, dnum / (n * M) + DIV_ULP * U * (nll.abs() + dnum / (n * M)))}
    if gate is not None:
        a2, b2 = gate_bce_fwd(gate, target, lens, mut="mask_le" if mut == "mask_le" else None)
        out["acc2"] = (a2, b2)
        out["gate"] = (a2 / n, b2 / n + DIV_ULP * U * (a2.abs() + b2) / n)
    return out


def flowtron_loss_bwd(z, gate, target, lens, sigma, inv_nm, inv_n, g_nll, g_gate, with_dls=True):
    """inv_nm, inv_n: acc[4], acc[5] as the forward left them (fp32 inputs).  dz = g_nll z inv_nm / sigma^2, dls = -g_nll inv_nm,
    dgate = g_gate inv_n (sigmoid(gate) - target), all 0 at padded frames.  Returns {"dz", "dls", "dgate"}."""
    T, B, M = z.shape
    m = frame_mask(lens, T)
    s32 = float(torch.tensor(sigma, dtype=torch.float32))
    out = {}
    if g_nll is not None:
        sc = float(g_nll) * float(inv_nm)
        dz = sc / (s32 * s32) * d(z) * m[:, :, None]
        out["dz"] = (dz, (4 + DIV_ULP) * U * dz.abs())             # g inv_nm; sigma^2; 1 / it; their product; times z
        if with_dls:
            dls = torch.full((T, B, M), -sc, dtype=F64, device=z.device) * m[:, :, None]
            out["dls"] = (dls, U * dls.abs())
    if g_gate is not None:
        out["dgate"] = gate_bce_bwd(gate, target, lens, float(g_gate), float(inv_n))
    return out


# ------------------------------------------------------------------------------------------------------------ colsum, act_bwd, eltwise, pad fill
def colsum(x):
    """x [rows, N] (a view of the strided matrix): out[n] = sum_r x[r][n]"""
    X = d(x)
    return X.sum(0), X.shape[0] * U * X.abs().sum(0)


def act_bwd(y, dy, act):
    """dpre = dy act'(pre) through the saved output y: tanh: dy (1 - y^2); relu: y > 0 ? dy : 0; sigmoid: dy y (1 - y); none: dy"""
    Y, G = d(y), d(dy)
    if act == ACT_TANH:
        f = 1 - Y * Y
        return G * f, G.abs() * U * (Y * Y + f.abs()) + U * (G * f).abs()
    if act == ACT_RELU:
        r = torch.where(Y > 0, G, torch.zeros_like(G))
        return r, torch.zeros_like(r)
    if act == ACT_SIGMOID:
        r = G * Y * (1 - Y)
        return r, 3 * U * r.abs()
    return G, torch.zeros_like(G)


def eltwise(a, b, op):
    """a + b (op 0) or a * b (op 1), each ONE correctly rounded fp32 operation: compared with torch.equal after .float() (a product of
    two fp32 is exact in float64; a sum is whenever the exponents are within 29 of each other, which `eltwise_inputs_ok` asserts)"""
    r = d(a) * d(b) if op else d(a) + d(b)
    return r, torch.zeros_like(r)


def eltwise_inputs_ok(a, b):
    lo = torch.minimum(a.abs(), b.abs())
    hi = torch.maximum(a.abs(), b.abs())
    return bool(((lo == 0) | (hi / lo.clamp(min=1e-45) < 2.0 ** 28)).all())


def pad_rows_fill(y, lens, T, B, mode):
    """y [T * B, cols]: rows (t, b) with t > lens[b] become 0 (mode 0) or a copy of row (lens[b], b) (mode 1); the rest stay"""
    Y = d(y).reshape(T, B, -1).clone()
    t = torch.arange(T, device=y.device)[:, None]
    ln = lens.clamp(min=0).long()
    pad = (t > ln[None, :])[:, :, None]
    src = Y[ln.clamp(max=T - 1), torch.arange(B, device=y.device)][None]
    Y = torch.where(pad, src.expand_as(Y) if mode else torch.zeros_like(Y), Y)
    Y = Y.reshape(T * B, -1)
    return Y, torch.zeros_like(Y)


# ------------------------------------------------------------------------------------------------------------ beta-binomial prior
def beta_binomial_prior(in_lens, out_lens, T, L, scaling):
    """prior[b, t, k] = BetaBinom.pmf(k; n = in_lens[b] - 1, a = s (t + 1), b = s (out_lens[b] - t)) for t < out_lens[b], k < in_lens[b],
    0 in the padding; s = the fp32 the ABI passes.  Relative bound: the fp32 rounding (2^-24) + the float64 error of seven lgamma terms
    at their magnitudes, and one fp32 subnormal absolutely."""
    s = float(torch.tensor(scaling, dtype=torch.float32))
    dev = in_lens.device
    P, Mo = in_lens.to(F64)[:, None, None], out_lens.to(F64)[:, None, None]
    t = torch.arange(T, dtype=F64, device=dev)[None, :, None]
    k = torch.arange(L, dtype=F64, device=dev)[None, None, :]
    ok = (t < Mo) & (k < P)
    n = P - 1
    kk = torch.where(ok, k.expand(ok.shape), torch.zeros((), dtype=F64, device=dev))
    a = s * (t + 1)
    b = torch.where(ok, s * (Mo - t), torch.ones((), dtype=F64, device=dev))
    nk = torch.where(ok, n - kk, torch.zeros((), dtype=F64, device=dev))
    n = torch.where(ok, n.expand(ok.shape), torch.zeros((), dtype=F64, device=dev))
    lg = torch.lgamma
    terms = [lg(n + 1), -lg(kk + 1), -lg(nk + 1), lg(kk + a), lg(nk + b), -lg(n + a + b), -(lg(a) + lg(b) - lg(a + b)).expand(ok.shape)]
    lp = sum(terms)
    mag = sum(x.abs() for x in terms) + (lg(a).abs() + lg(b).abs() + lg(a + b).abs())
    ref = torch.exp(lp) * ok
    rel = 2.0 ** -24 + (LGAMMA_ULP64 + 10) * 2.0 ** -53 * mag + 4 * 2.0 ** -53
    return ref, (ref * rel + FLT_SUBNORMAL) * ok


# ------------------------------------------------------------------------------------------------------------ RAdam, one step
def radam_step(p, g, m, v, *, gnorm_sq, clip, lr, beta1, beta2, eps, weight_decay, step_size, rectified, mut=None, threads=None):
    """One ft_radam_step with a finite norm: cs = min(1, clip / (sqrt(gnorm_sq) + 1e-6)) (clip > 0), g' = g cs, v = b2 v + (1 - b2) g'^2,
    m = b1 m + (1 - b1) g', p -= wd lr p, p -= step_size (rectified ? m / (sqrt(v) + eps) : m).  The coefficients are the doubles rounded
    to fp32 once (header).  Returns {"p", "m", "v"}."""
    f = lambda val: float(torch.tensor(val, dtype=torch.float32))
    b1, b2, o1, o2, ep, ss, wl = f(beta1), f(beta2), f(1.0 - beta1), f(1.0 - beta2), f(eps), f(step_size), f(weight_decay * lr)
    cs, rcs = 1.0, 0.0
    if gnorm_sq is not None and clip > 0:
        c = f(clip) / (math.sqrt(f(gnorm_sq)) + f(1e-6))
        if c < 1.0:
            cs, rcs = c, (SQRT_ULP + 1 + DIV_ULP) * U
    P, G, M0, V0 = d(p), d(g), d(m), d(v)
    gi = G * cs
    rg = rcs + (U if cs != 1.0 else 0.0)                           # relative error of g'
    vi = o2 * gi * gi + b2 * V0
    dvi = o2 * gi * gi * (2 * rg + 2 * U) + U * b2 * V0.abs() + U * vi.abs()
    mi = o1 * gi + b1 * M0
    dmi = o1 * gi.abs() * (rg + U) + U * b1 * M0.abs() + U * mi.abs()
    pi, dpi = P, torch.zeros_like(P)
    if wl != 0.0:
        pi = P - wl * P
        dpi = U * (P.abs() + (wl * P).abs())
    if rectified:
        sq = torch.sqrt(vi)
        dsq = sq * SQRT_ULP * U + torch.where(vi > 0, dvi / (2 * torch.sqrt((vi - dvi).clamp(min=1e-300))), torch.sqrt(dvi))
        den = sq + ep
        dden = dsq + U * den
        q = mi / den
        dq = dmi / den + q.abs() * dden / (den - dden).clamp(min=1e-300) + DIV_ULP * U * q.abs()
    else:
        q, dq = mi, dmi
    upd = ss * q
    dupd = ss * dq + U * upd.abs()
    pn = pi - upd
    dpn = dpi + dupd + U * (pi.abs() + upd.abs() + dpi + dupd)
    if mut == "pass2":
        first = first_pass(P.shape, threads, P.device)
        pn, mi, vi = torch.where(first, pn, P), torch.where(first, mi, M0), torch.where(first, vi, V0)
    return {"p": (pn, dpn), "m": (mi, dmi), "v": (vi, dvi)}


# ------------------------------------------------------------------------------------------------------------ fp32 emulations (CPU tests)
ORDERS = ("seq", "lanes4", "lanes16", "lanes64", "rev")


def emu_sum(t32, order="seq"):
    """fp32 sum over dim 0 of t32 [n, ...] in a stated order: sequential, reversed, or over k lanes (lane j adds rows j, j + k, ... in
    sequence; the lanes are then added in lane order) -- the shapes a kernel's per-thread loop and its lane reduction can take"""
    n = t32.shape[0]
    zero = torch.zeros(t32.shape[1:], dtype=torch.float32)
    if n == 0:
        return zero
    if order in ("seq", "rev"):
        acc = zero.clone()
        for i in (range(n - 1, -1, -1) if order == "rev" else range(n)):
            acc = acc + t32[i]
        return acc
    k = int(order[5:])
    trips = -(-n // k)
    pad = torch.cat([t32, torch.zeros((trips * k - n,) + tuple(t32.shape[1:]), dtype=torch.float32)]).reshape((trips, k) + tuple(t32.shape[1:]))
    lanes = torch.zeros((k,) + tuple(t32.shape[1:]), dtype=torch.float32)
    for i in range(trips):
        lanes = lanes + pad[i]
    acc = zero.clone()
    for j in range(k):
        acc = acc + lanes[j]
    return acc


SPLITS = ("fwd", "rev", "shuffle")


def emu_flat_sum(t32, threads=1024, block=256, split="fwd", seed=0):
    """fp32 grid-stride sum of the flat t32: thread i adds elements i, i + threads, ... in sequence, the threads of a block are added
    pairwise (a tree), the per-block partials in forward, reversed or shuffled order (atomics)"""
    t = t32.reshape(-1)
    n = t.numel()
    passes = -(-n // threads)
    pad = torch.cat([t, torch.zeros(passes * threads - n, dtype=torch.float32)]).reshape(passes, threads)
    th = torch.zeros(threads, dtype=torch.float32)
    for i in range(passes):
        th = th + pad[i]
    blk = th.reshape(-1, block)
    w = block
    while w > 1:
        w //= 2
        blk = blk[:, :w] + blk[:, w:2 * w]
    parts = blk[:, 0]
    idx = list(range(parts.numel()))
    if split == "rev":
        idx = idx[::-1]
    elif split == "shuffle":
        idx = torch.randperm(len(idx), generator=gen(seed)).tolist()
    acc = torch.zeros((), dtype=torch.float32)
    for i in idx:
        acc = acc + parts[i]
    return acc
