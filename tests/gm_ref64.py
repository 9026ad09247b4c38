"""Float64 restatement of the Gaussian-mixture entry points of include/flowtron_hip.h (csrc/mixture.hip): mixture NLL forward and
backward, time pooling, row softmax, component sampler -- each with a per-element error bound that follows the kernel's own fp32
operation chain (imported by tests/test_mixture_cpu.py and tests/test_gpu_mixture.py, not collected).  Plain torch on whatever device
the inputs live on; nothing here calls the project's kernels.  Every function returns (reference, bound) in float64 (a dict of such
pairs where an entry point has several outputs); bound 0 = the element must come back EQUAL (padding, copies).

Conventions, as in tests/elementwise_ref64.py: u = U = 2^-23, one whole ulp per rounding (a truncating implementation passes too);
device math functions at the OpenCL full-profile limits the ROCm device library implements without fast-math (expf <= 3 ulp, logf <= 3,
x / y <= 2.5); a value known to within +-e enters a product with magnitude (|v| + e); a result that may underflow gets the floor FLT_MIN.
Reductions: a sum whose every term passes through at most D fp32 additions, each rounding a partial sum no larger than sum |terms|, is
off by at most D u sum |terms| plus the terms' own errors.  D is read off the kernel's layout (NT 256 threads, FPT 8 frames per thread,
R = 256 / M frame rows per workgroup, wave_sum = 6 levels, 4 waves per workgroup) and stated at each use -- the ordered two-stage
reductions of mixture.hip are what makes D small; a kernel that summed in another layout would need its own count."""
import math

import torch

U = 2.0 ** -23
F64 = torch.float64
EXP_ULP, LOG_ULP, DIV_ULP = 3.0, 3.0, 2.5
FLT_MIN = 2.0 ** -126
NT, FPT, WAVE_LEVELS, WAVES = 256, 8, 6, 4
SHARP = 1.0                                                     # a wrong reference must lie more than SHARP bounds away


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


def frame_mask(lens, T):
    """[T, B] bool: t < min(lens[b], T)"""
    return torch.arange(T, device=lens.device)[:, None] < lens.clamp(0, T)[None, :]


def _prod_err(*pairs):
    """(|v_1| + e_1) ... (|v_k| + e_k) - |v_1 ... v_k| and the first product: the error of an exact product of values known to +-e_i"""
    hi, lo = None, None
    for v, e in pairs:
        hi = (v.abs() + e) if hi is None else hi * (v.abs() + e)
        lo = v.abs() if lo is None else lo * v.abs()
    return hi - lo, hi


def _exp_err(val, darg):
    """error of expf(arg) whose argument is off by at most darg: exp(arg) (e^darg - 1) for the argument, EXP_ULP ulps of the (larger)
    result for the function, FLT_MIN where the result may be flushed"""
    g = torch.expm1(darg.clamp(max=80.0))
    return val * g + EXP_ULP * U * val * (1.0 + g) + FLT_MIN


# ------------------------------------------------------------------------------------------------------------ the element chain
def _chain(z, mean, log_var, prob):
    """per (t, b, m, c): the chain of mixture.hip's load_consts / comp_u / mixture_lse in float64 with the error of every step.
    z [T,B,M], mean / log_var [Bm,M,C], prob [B,C] -> dict of [T,B,M,C] (and [T,B,M]) float64 tensors."""
    Z, MU, LV, P = d(z)[..., None], d(mean)[None], d(log_var)[None], d(prob)[None, :, None, :]
    inv = torch.exp(-LV)                                        # expf(-lv): EXP_ULP ulps (the negation is exact)
    a, da = -0.5 * inv, EXP_ULP * U * 0.5 * inv                 # a = -0.5 inv: an exact scaling
    h = -0.5 * LV                                               # exact
    lp = torch.log(P)
    dlp = LOG_ULP * U * lp.abs() + FLT_MIN                      # logf(prob)
    dd_ = Z - MU
    ddd = U * dd_.abs()                                         # d = z - mean: one rounding
    d2 = dd_ * dd_
    e2, hi2 = _prod_err((dd_, ddd), (dd_, ddd))
    dd2 = e2 + U * hi2                                          # d2 = d * d: the factors' errors, one rounding
    u_ = a * d2 + h
    ea, hia = _prod_err((a, da), (d2, dd2))
    du = ea + U * (u_.abs() + ea)                               # u = fma(a, d2, h): the product's error, ONE rounding of the sum (h exact)
    e_ = lp + u_
    de = dlp + du + U * (e_.abs() + dlp + du)                   # e = lp + u
    mx = e_.max(-1, keepdim=True)[0]
    dmx = de.max(-1, keepdim=True)[0]
    # The kernel shifts by mh, the largest COMPUTED e_c, which lies within dmx of mx.  l = mh + log sum_c exp(e_c - mh) holds exactly
    # for any shift, so the shift carries no error of its own: against s' = sum_c exp(e_c - mh) = s exp(mx - mh) the computed sum has
    # the RELATIVE error derived below for s (a common factor within e^dmx of 1 on every term), and l = mx + log s = mh + log s'.
    arg = e_ - mx
    darg = de + U * (arg.abs() + de + dmx)                      # e_c - mh: e_c's error, one rounding of a difference within dmx of arg
    t_ = torch.exp(arg)
    dt = _exp_err(t_, darg)
    s = t_.sum(-1)
    C = t_.shape[-1]
    ds = dt.sum(-1) + C * U * (t_ + dt).sum(-1)                 # sequential sum over c: D = C
    logs = torch.log(s)
    # log s' = log s + (mx - mh), |mx - mh| <= dmx: logf's ulps are taken of the larger magnitude; s' >= e^-dmx (its largest term)
    dlogs = ds / (s - ds).clamp(min=0.5) + LOG_ULP * U * (logs.abs() + dmx[..., 0]) + FLT_MIN
    l = mx[..., 0] + logs
    dl = dlogs + U * (l.abs() + dlogs)                          # mh + log s': one rounding
    return dict(Z=Z, P=P, a=a, da=da, inv=inv, d=dd_, dd=ddd, d2=d2, dd2=dd2, u=u_, du=du, l=l, dl=dl)


def chunk_geometry(T, M):
    R = NT // M
    CH = R * FPT
    return R, CH, -(-T // CH)


# ------------------------------------------------------------------------------------------------------------ mixture NLL forward
def mixture_nll_fwd(z, mean, log_var, prob, lens, log_s=(), extra_frame=False):
    """loss = -(sum_valid l + sum_f sum_valid log_s_f) / (n M), l = log sum_c prob_c exp(-(z - mean_c)^2 / (2 exp(lv_c))) / sqrt(exp(lv_c)).
    Padded frames are masked BEFORE anything is summed (NaN there does not reach the result).  extra_frame: the wrong reference that
    counts one frame past every length below T.  -> (loss, bound), float64 scalars."""
    T, B, M = z.shape
    ln = lens.clamp(0, T)
    if extra_frame:
        ln = (ln + 1).clamp(max=T)
    m = frame_mask(ln, T)[:, :, None]
    zz = torch.where(m, z, torch.zeros((), dtype=z.dtype, device=z.device))
    k = _chain(zz, mean, log_var, prob)
    zero = torch.zeros((), dtype=F64, device=z.device)
    l, dl = torch.where(m, k["l"], zero), torch.where(m, k["dl"], zero)
    ls = [torch.where(m, d(x), zero) for x in log_s]
    total = -(l.sum() + sum(x.sum() for x in ls))
    mag = l.abs().sum() + sum(x.abs().sum() for x in ls)
    F_ = len(ls)
    _, _, nk = chunk_geometry(T, M)
    # additions a term passes through: v = l + ls_1 + .. (F), nl -= v over the thread's FPT frames, wave_sum, the workgroup's 4 waves;
    # finalize: ceil(nk B / 256) partials per thread, wave_sum, 4 waves
    D = FPT * (F_ + 1) + WAVE_LEVELS + WAVES + -(-nk * B // NT) + WAVE_LEVELS + WAVES
    dtotal = dl.sum() + D * U * (mag + dl.sum())
    nm = float(ln.sum()) * M                                    # n M: integers below 2^24, exact in fp32
    loss = total / nm
    return loss, dtotal / nm + DIV_ULP * U * loss.abs()


# ------------------------------------------------------------------------------------------------------------ mixture NLL backward
def mixture_nll_bwd(z, mean, log_var, prob, lens, g=1.0, has_ls=True):
    """gradients of g * loss: {"dz", "dls" [T,B,M]; "dmean", "dlog_var" [B,M,C] (per utterance also for Bm = 1); "dprob" [B,C]}
    -> (ref, bound).  With r_c = prob_c q_c, q_c = exp(u_c - l), sc = g / (n M):
      dz = sc sum_c r_c d / var_c ; dls = -sc ; dmean_c = -sc sum_t r_c d / var_c ; dlog_var_c = sc sum_t r_c (1/2 + a_c d^2) ;
      dprob_c = -sc sum_{t,m} q_c ; all zero at padded frames."""
    T, B, M = z.shape
    C = prob.shape[1]
    ln = lens.clamp(0, T)
    m = frame_mask(ln, T)[:, :, None]
    m4 = m[..., None]
    zz = torch.where(m, z, torch.zeros((), dtype=z.dtype, device=z.device))
    k = _chain(zz, mean, log_var, prob)
    zero = torch.zeros((), dtype=F64, device=z.device)
    nm = float(ln.sum()) * M
    sc = float(g) / nm
    dsc = (DIV_ULP + 1.0) * U * abs(sc)                        # acc[4] = 1 / (n M): a division; sc = g * acc[4]: one rounding
    arg = k["u"] - k["l"][..., None]
    darg = k["du"] + k["dl"][..., None] + U * (arg.abs() + k["du"] + k["dl"][..., None])       # u - l
    q = torch.exp(arg)
    dq = _exp_err(q, darg)
    P = k["P"].expand_as(q)
    r = P * q
    dr = P * dq + U * P * (q + dq)                              # rc = p * q (p an input: exact)
    inv, dinv = k["inv"].expand_as(q), 2.0 * k["da"].expand_as(q)                              # inv = -2 a: exact scaling of a
    w = r * k["d"] * inv
    ew, hiw = _prod_err((r, dr), (k["d"], k["dd"]), (inv, dinv))
    dw = ew + 2.0 * U * hiw                                     # (rc * d) * inv: two roundings
    f = k["a"] * k["d2"] + 0.5
    ef, _ = _prod_err((k["a"].expand_as(q), k["da"].expand_as(q)), (k["d2"], k["dd2"]))
    df = ef + U * (f.abs() + ef)                                # fma(a, d2, 0.5)
    v = r * f
    ev, hiv = _prod_err((r, dr), (f, df))
    dv = ev + U * hiv                                           # rc * f
    w, dw, v, dv, q, dq = (torch.where(m4, x, zero) for x in (w, dw, v, dv, q, dq))
    hw, hv, hq = w.abs() + dw, v.abs() + dv, q + dq
    R, CH, nk = chunk_geometry(T, M)

    def scaled(sm, dsm):
        """sc * sm: sm known to +-dsm, sc to +-dsc, one rounding"""
        out = sc * sm
        return out, abs(sc) * dsm + dsc * (sm.abs() + dsm) + U * (out.abs() + abs(sc) * dsm)

    res = {}
    # dz: dza += w_c sequentially over c (D = C)
    res["dz"] = scaled(w.sum(-1), dw.sum(-1) + C * U * hw.sum(-1))
    res["dz"] = (res["dz"][0], torch.where(m, res["dz"][1], zero))
    if has_ls:
        res["dls"] = (torch.where(m, torch.full_like(k["l"], -sc), zero), torch.where(m, torch.full_like(k["l"], dsc), zero))
    # dmean, dlog_var: a thread adds its FPT frames, the workgroup its R frame rows, the second kernel the utterance's nk chunks
    D = FPT + R + nk
    res["dmean"] = scaled(-w.sum(0), dw.sum(0) + D * U * hw.sum(0))
    res["dlog_var"] = scaled(v.sum(0), dv.sum(0) + D * U * hv.sum(0))
    # dprob: FPT frames per thread, wave_sum, 4 waves, nk chunks
    D = FPT + WAVE_LEVELS + WAVES + nk
    res["dprob"] = scaled(-q.sum((0, 2)), dq.sum((0, 2)) + D * U * hq.sum((0, 2)))
    return res


# ------------------------------------------------------------------------------------------------------------ time pooling
def time_pool_fwd(x, lens):
    """y[b] = sum_{t < lens[b]} x[t, b] / max_b lens[b] (lengths clamped to 0 ..= T).  x [T,B,W]."""
    T = x.shape[0]
    ln = lens.clamp(0, T)
    m = frame_mask(ln, T)[:, :, None]
    X = torch.where(m, d(x), torch.zeros((), dtype=F64, device=x.device))
    mx = float(ln.max())
    y = X.sum(0) / mx
    # four time slices per channel: ceil(len / 4) sequential additions in a slice, then the 3 that join the slices
    D = (-(-ln // 4) + 3).to(F64)[:, None]
    return y, D * U * X.abs().sum(0) / mx + DIV_ULP * U * y.abs()


def time_pool_bwd(dy, lens, T):
    """dx[t, b] = dy[b] / max_b lens[b] at t < lens[b], 0 beyond"""
    ln = lens.clamp(0, T)
    m = frame_mask(ln, T)[:, :, None]
    dx = (d(dy) / float(ln.max()))[None].expand(T, -1, -1)
    zero = torch.zeros((), dtype=F64, device=dy.device)
    return torch.where(m, dx, zero), torch.where(m, DIV_ULP * U * dx.abs(), zero)


# ------------------------------------------------------------------------------------------------------------ row softmax
def softmax_rows_fwd(x):
    X = d(x)
    arg = X - X.max(1, keepdim=True)[0]                         # (the largest fp32 value is found exactly)
    e = torch.exp(arg)
    de = _exp_err(e, U * arg.abs())                             # x - max: one rounding
    s = e.sum(1, keepdim=True)
    ds = de.sum(1, keepdim=True) + WAVE_LEVELS * U * (e + de).sum(1, keepdim=True)             # wave_sum
    y = e / s
    return y, y * (de / e.clamp(min=FLT_MIN) + ds / (s - ds)) + DIV_ULP * U * y + FLT_MIN


def softmax_rows_bwd(y, dy):
    """dx = y (dy - sum_c y_c dy_c), y as given (the forward's fp32 result is the kernel's input)"""
    Y, G = d(y), d(dy)
    p = Y * G
    S = p.sum(1, keepdim=True)
    dS = (U * p.abs()).sum(1, keepdim=True) + WAVE_LEVELS * U * ((1 + U) * p.abs()).sum(1, keepdim=True)   # the products' roundings, wave_sum
    t = G - S
    dt = dS + U * (t.abs() + dS)
    dx = Y * t
    return dx, Y.abs() * dt + U * Y.abs() * (t.abs() + dt)


# ------------------------------------------------------------------------------------------------------------ sampler
def mixture_sample(mean, log_var, rows, comp, eps, sigma):
    """out[s,m,t] = mean[rows[s],m,comp[s]] + sigma exp(log_var[..] / 2) eps[s,m,t]; eps None: the means (equal)"""
    mu = d(mean)[rows.long(), :, comp.long()][:, :, None]       # [S,M,1]
    if eps is None:
        return mu.clone(), torch.zeros_like(mu)
    lv = d(log_var)[rows.long(), :, comp.long()][:, :, None]
    e = torch.exp(0.5 * lv)                                     # 0.5 lv exact; expf
    sd = float(sigma) * e
    dsd = (EXP_ULP + 1.0) * U * sd                              # sigma * e: one rounding
    out = mu + sd * d(eps)
    return out, dsd * d(eps).abs() + U * (out.abs() + dsd * d(eps).abs())                      # fma: one rounding


# ------------------------------------------------------------------------------------------------------------ the reference's formula
def reference_formula_nll(z, mean, log_var, prob, lens, log_s):
    """flowtron.py:217-235 term by term in float64 (the linear-domain form the reference evaluates): what mixture_nll_fwd must equal"""
    T, B, M = z.shape
    mask = frame_mask(lens, T)[:, :, None, None].to(F64)
    Z, MU, LV, P = d(z)[..., None], d(mean)[None], d(log_var)[None], d(prob)[None, :, None]
    _z = -(Z - MU) ** 2 / (2 * torch.exp(LV))
    _zmax = _z.max(dim=3, keepdim=True)[0]
    _z = P * torch.exp(_z - _zmax) / torch.sqrt(torch.exp(LV))
    _z = _zmax + torch.log(torch.sum(_z, dim=3, keepdim=True))
    nll = -torch.sum(mask * _z)
    total = sum(torch.sum(d(x) * mask[..., 0]) for x in log_s)
    return (nll - total) / (mask.sum() * M)


def bf16_ulp(x):
    """one bf16 ulp of |x| (8 significand bits): 2^(floor(log2 |x|) - 7)"""
    return 2.0 ** (math.floor(math.log2(abs(float(x)))) - 7)
