"""Float64 references of the alignment path's two kernels, with per-element error bounds (imported by the tests, not collected).

Plain torch; runs on the CPU or, for the large shapes, in float64 on the device.  Nothing here calls the project's kernels.

  attention (csrc/attention.hip, oracle.flowtron_oracle.attention / reference flowtron.py:544-583)
      e[b,t,l] = sum_a v[a] tanh(Q[t,b,a] + K[l,b,a]) / temp        (l < in_lens[b]; -inf beyond)
      p = softmax_l(e);  no prior: attn = p, logprob = log(p + 1e-8)
                         prior:    u = log(p + 1e-20) + log(prior + 1e-20), logprob = u, attn = softmax_{l < len}(u)
  attention backward: de (the kernel's de_work: dL/d(sum_a v tanh), i.e. 1/temp included), then from a GIVEN de
      dQ[t,b,a] = v[a] sum_l de (1 - tanh^2),  dK[l,b,a] = v[a] sum_t de (1 - tanh^2),  dv[a] = sum_{b,t,l} de tanh
  attention-CTC (csrc/ctc.hip, oracle.attention_ctc_loss / reference flowtron.py:155-182): explicit alpha / beta recursions over
      the 2K+1 states of the trivial target 1..K with a blank column of logit `blank`, log-softmax over the K+1 classes per frame.

Each stage is checked on its own fp32 inputs, like the recurrence replay: the backward's reference is fed the kernel's own attn /
p_save, and dQ / dK / dv are fed the kernel's own de.  A stage's bound therefore covers that stage's arithmetic alone.

Unit: U = 2^-24, the fp32 unit roundoff; one ulp of the hardware transcendentals (v_exp_f32, v_rcp_f32, v_log_f32) and of ocml's
expf / logf is taken as 2 U relative.  Every constant below counts roundings on the longest path of the kernel's code."""
import math

import torch

U = 2.0 ** -24
LN2 = math.log(2.0)
C2 = 2.0 * math.log2(math.e)          # the kernel folds tanh's argument scale into q' = C2 q, k' = C2 k (attention.hip C2)
EXP_SAFE = 60.0                        # |q'| or |k'| above this: the sum form of r (attention.hip EXP_SAFE)
TT = 32                                # query rows per workgroup / per backward tile
AC = 64                                # a-chunk of the forward
P_FLOOR = 2.0 ** -126                  # expf(x) flushed or subnormal: absolute error below the smallest normal
C_EXP = 4      # relative error of X = 2^q' 2^k' (two v_exp_f32), or of 2^(q'+k') (one)
C_RD = 3       # r = rcp(fma(Eq, Ek, 1)): v_rcp_f32 plus the fma's rounding
C_ARG = 3      # the argument: C2 rounded to fp32, the products C2 q and C2 k, and the sum form's q' + k'
C_T = 3        # e = (vsum - 2 acc) * inv_temp: the subtraction, the product, 1/temp rounded on the host
C_SM = 10      # one softmax element beyond its summation: e - m, expf, the division, the pre-filter ordering slack
C_LOGF = 3     # logf(x + eps): the argument's rounding, eps rounded to fp32, logf's ulp (in units of U |log|: see bound_logprob)
C_DP = 5       # no-prior dp = dattn + dlogprob / (p + 1e-8f): p + eps, eps's own rounding, the division, the add, p * dp
C_DU = 3       # prior du = attn (dattn - s1) + dlogprob: subtraction, product, add
C_X = 4        # prior p * (du / (p + 1e-20f)): p + eps, eps's rounding, the division, the product
C_LSE3 = 16    # lse3 / lse2 of ctc.hip beyond the max of its inputs' errors: three x*log2e roundings and v_exp_f32 (<= 3 U each on
#                the dominant term, and d e^-d <= 1/e on the others), two adds, v_log_f32 on [1, 3] (<= 2 U * log2 3) and its scale


def _wsum_depth(n):
    """roundings on the longest path of a 64-lane strided sum of n terms (per-lane sequential, then a 6-level shuffle tree)"""
    return -(-n // 64) + 6


def softmax_err(a, d):
    """|a' - a| for a' = softmax(log a + delta) with |delta_l| <= d_l (rigorous, first order d_l + sum_m a_m d_m):
    a'_l / a_l = e^{delta_l} / sum_m a_m e^{delta_m}, and sum_m a_m e^{delta_m} lies in [1/(1 + sum a (e^d - 1)), 1 + sum a (e^d - 1)]."""
    s = torch.log1p((a * torch.expm1(d)).sum(-1, keepdim=True))
    return a * torch.expm1(d + s)


def _log_eps_err(x, dx, eps):
    """|log(x' + eps) - log(x + eps)| for |x' - x| <= dx (log is monotone): log((x + eps) / (x + eps - dx))"""
    frac = (dx / (x + eps)).clamp(max=1.0)
    return -torch.log1p(-frac)


# ------------------------------------------------------------------------------------------------------------------ attention
def sum_form_rows(Q):
    """[T,B] bool: the kernel's rule, evaluated in fp32 as the kernel does: some |C2 q| > EXP_SAFE in the row"""
    return ~((torch.tensor(C2, dtype=torch.float32) * Q.float().to(Q.device)).abs() <= EXP_SAFE).all(-1)


def sum_form_keys(K, in_lens):
    """[L,B] bool: valid key l of utterance b has some |C2 k| > EXP_SAFE"""
    Lk = K.shape[0]
    big = ~((torch.tensor(C2, dtype=torch.float32) * K.float()).abs() <= EXP_SAFE).all(-1)
    valid = torch.arange(Lk, device=K.device)[:, None] < in_lens.to(K.device).long()[None, :]
    return big & valid


def _r_and_err(x, qk_abs):
    """r = 1 / (e^{2x} + 1) (the kernel's r = 1 / (2^{C2 x} + 1); tanh = 1 - 2r, 1 - tanh^2 = 4 r (1 - r)) and a bound on the kernel's
    |dr|.  r = 1/(1 + X) with X = 2^{x'}: X carries a relative error eps_X = C_EXP U (the exp2s) + ln2 C_ARG U (|q'| + |k'|) (an
    argument error dx' moves X by ln2 X dx'); dr / r = -X/(1+X) dX/X = -(1 - r) eps_X, and the fma and v_rcp_f32 add C_RD U r.
    Below the normal range fp32 holds no r at all: where 2^x' overflows (x' > 128, the sum form) the kernel's r is exactly 0, so
    |dr| also carries P_FLOOR."""
    r = torch.sigmoid(-2.0 * x)
    s = torch.sigmoid(2.0 * x)                       # 1 - r without cancellation
    eps_x = C_EXP * U + LN2 * C_ARG * U * C2 * qk_abs
    return r, s, r * (s * eps_x + C_RD * U) + P_FLOOR


def _chunk_rows(B, L, A, dev):
    """query rows per chunk of the [B, rows, L, A] float64 temporaries (~24 MB each on the CPU, ~400 MB on the device)"""
    return max(1, int((5e7 if dev.type == "cuda" else 3e6) // max(1, B * L * A)))


def attention_fwd(Q, K, v, in_lens, prior=None, temperature=1.0, bounds=True):
    """float64 forward.  Q [T,B,A], K [L,B,A], v [A] (any dtype; computed in float64 on Q's device), in_lens [B], prior [B,T,L] or None.
    Returns dict(e, p, attn, logprob[, delta]) as [B,T,L]; e is -inf at l >= in_lens[b].  delta (bounds=True): a bound on the kernel's
    score error of each element BEYOND a shift common to the whole row (see score_err)."""
    dev = Q.device
    Qd, Kd, vd = Q.double(), K.double().to(dev), v.double().reshape(-1).to(dev)
    T, B, A = Qd.shape
    Lk = Kd.shape[0]
    lens = in_lens.to(dev).long().clamp(max=Lk)
    valid = torch.arange(Lk, device=dev)[None, :] < lens[:, None]               # [B,L]
    Kd = torch.where(valid.t()[..., None], Kd, torch.zeros((), dtype=torch.float64, device=dev))   # padding (even NaN) never read
    Qb, Kb = Qd.transpose(0, 1), Kd.transpose(0, 1)                               # [B,T,A], [B,L,A]
    e = torch.empty(B, T, Lk, dtype=torch.float64, device=dev)
    delta = torch.empty_like(e) if bounds else None
    if bounds:
        va = vd.abs()
        n_e = score_depth(Q, K, in_lens, A)                                       # [B]
        qa, ka = Qb.abs(), Kb.abs()
    tc = _chunk_rows(B, Lk, A, dev)
    for t0 in range(0, T, tc):
        x = Qb[:, t0:t0 + tc, None, :] + Kb[:, None, :, :]                        # [B,tc,L,A]
        e[:, t0:t0 + tc] = torch.tanh(x) @ vd
        if bounds:
            r, _, dr = _r_and_err(x, qa[:, t0:t0 + tc, None, :] + ka[:, None, :, :])
            del x
            delta[:, t0:t0 + tc] = (2.0 * (dr @ va) + n_e[:, None, None] * U * 2.0 * (r @ va)) / temperature
            del r, dr
    e = e / temperature
    if bounds:
        delta = delta + C_T * U * e.abs()
    e = e.masked_fill(~valid[:, None, :], -math.inf)
    p = torch.softmax(e, 2)
    out = dict(e=e, p=p, valid=valid, lens=lens, temperature=float(temperature), prior=None)
    if prior is not None:
        pr = prior.float().double().to(dev)              # the prior is read as fp32 (oracle: attn_prior.float(); the kernel)
        u = torch.log(p + 1e-20) + torch.log(pr + 1e-20)
        out["logprob"] = u
        out["attn"] = torch.softmax(u.masked_fill(~valid[:, None, :], -math.inf), 2)
        out["prior"] = pr
    else:
        out["attn"] = p
        out["logprob"] = torch.log(p + 1e-8)
    if bounds:
        out["delta"] = torch.where(valid[:, None, :], delta, torch.zeros((), dtype=torch.float64, device=dev))
    return out


def score_depth(Q, K, in_lens, A):
    """[B] float: roundings on the longest path of the kernel's sum_a v r.  Product form: per lane, a chunk's 16 float4 steps of two
    packed FMAs (32), the lane pair's add, one add per chunk into acc (ceil(A/64)), +1.  Sum form (an utterance with some
    |C2 q| or |C2 k| > 60): acc += (four products), 16 steps per chunk, carried across chunks: A/4 + 5."""
    dev = Q.device
    lens = in_lens.to(dev).long()
    big = sum_form_rows(Q).any(0) | sum_form_keys(K.to(dev), lens).any(0)
    prod = 34.0 + -(-A // AC)
    return torch.where(big, torch.full_like(lens, A // 4 + 5 + 2, dtype=torch.float64),
                       torch.full_like(lens, prod, dtype=torch.float64))


def score_err(ref):
    """Bound on the kernel's scores e' beyond a common shift per (b, t) row, which the softmax removes.
      e' temp = vsum - 2 sum_a v r' with both sums in fp32.  vsum = sum_a v[a] is summed in the SAME order for every (t, l) of a row
      (every thread walks all of v), so its error is one constant per row.  The rest, per element:
        2 sum_a |v| |dr_a|                 the r of every a, see _r_and_err;
        n_e U 2 sum_a |v| r_a              the fp32 sum of v r (depth n_e, score_depth);
        C_T U |e|                          vsum - 2 acc, * inv_temp, and 1/temp rounded.
    (The |q| + |k| of C2 q / C2 k rounding enters through eps_X.)"""
    return ref["delta"]


def bound_p(ref):
    """p = softmax_l(e'): the score errors through softmax_err, plus the softmax's own arithmetic: e - m rounded (U |e - max|,
    relative in expf), expf's ulp, the 64-lane sum (depth ceil(len/64) + 6), the division: relative U (|e - max| + depth + C_SM);
    plus P_FLOOR for expf results below the normal range.  0 at l >= len (the kernel writes exact zeros there)."""
    e, p, valid = ref["e"], ref["p"], ref["valid"]
    emax = e.amax(2, keepdim=True)
    depth = torch.tensor([_wsum_depth(int(n)) for n in ref["lens"].tolist()], dtype=torch.float64, device=e.device)
    gap = torch.where(valid[:, None, :], (e - emax).abs(), torch.zeros((), dtype=torch.float64, device=e.device))
    d = ref["delta"] + U * (gap + depth[:, None, None] + C_SM)
    return torch.where(valid[:, None, :], softmax_err(p, d) + P_FLOOR, torch.zeros((), dtype=torch.float64, device=e.device))


def _logu_err(ref):
    """prior posterior's u = logf(p + 1e-20f) + logf(prior + 1e-20f): the p error through log(p + eps) (exact, _log_eps_err), and per
    logf: C_LOGF U (1 + |log|) -- argument rounding and eps rounded (U each, absolute after the log), logf's ulp (2 U |log|) --, plus
    the add (U |u|)."""
    p, pr = ref["p"], ref["prior"]
    lp, lq = torch.log(p + 1e-20), torch.log(pr + 1e-20)
    return (_log_eps_err(p, bound_p(ref), 1e-20) + C_LOGF * U * (2.0 + lp.abs() + lq.abs()) + U * (lp + lq).abs())


def bound_logprob(ref):
    """no prior: logf(p + 1e-8f): the p error through log (exact), then C_LOGF U (1 + |log|).  prior: see _logu_err."""
    if ref["prior"] is None:
        p = ref["p"]
        return _log_eps_err(p, bound_p(ref), 1e-8) + C_LOGF * U * (1.0 + torch.log(p + 1e-8).abs())
    return _logu_err(ref)


def bound_attn(ref):
    """no prior: attn = p (bound_p).  prior: softmax_{l < len}(u') with |u' - u| <= _logu_err through softmax_err, plus the second
    softmax's own arithmetic as in bound_p."""
    if ref["prior"] is None:
        return bound_p(ref)
    a, valid, lu = ref["attn"], ref["valid"], ref["logprob"]
    z = torch.zeros((), dtype=torch.float64, device=a.device)
    lu = lu.masked_fill(~valid[:, None, :], -math.inf)
    gap = torch.where(valid[:, None, :], (lu - lu.amax(2, keepdim=True)).abs(), z)
    depth = torch.tensor([_wsum_depth(int(n)) for n in ref["lens"].tolist()], dtype=torch.float64, device=a.device)
    d = torch.where(valid[:, None, :], _logu_err(ref), z) + U * (gap + depth[:, None, None] + C_SM)
    return torch.where(valid[:, None, :], softmax_err(a, d) + P_FLOOR, z)


def attention_de(attn, p_save, dattn, dlogprob, in_lens, temperature, prior=True):
    """float64 de = dL/d(sum_a v tanh) (1/temp included) from GIVEN attn [B,T,L] and p_save (the forward's p; prior case), dattn and
    dlogprob (or None).  Returns (de, bound): the bound covers the kernel's arithmetic on these same fp32 inputs (docstrings inline).
      no prior: dp = dattn + dlogprob / (p + 1e-8);  s2 = sum_{l<len} p dp;  de = p (dp - s2) / temp
      prior:    s1 = sum attn dattn;  du = attn (dattn - s1) + dlogprob;  x = du / (p + 1e-20);  s2 = sum p x;  de = p (x - s2) / temp"""
    dev = attn.device
    P = attn.double()
    Lk = P.shape[2]
    lens = in_lens.to(dev).long().clamp(max=Lk)
    valid = (torch.arange(Lk, device=dev)[None, :] < lens[:, None])[:, None, :]
    z = torch.zeros((), dtype=torch.float64, device=dev)
    depth = torch.tensor([_wsum_depth(int(n)) for n in lens.tolist()], dtype=torch.float64, device=dev)[:, None, None]
    da = torch.where(valid, dattn.double(), z)
    dl = torch.where(valid, dlogprob.double(), z) if dlogprob is not None else torch.zeros_like(P)
    it = 1.0 / temperature
    if not prior:
        P = torch.where(valid, P, z)
        dp = da + dl / (P + 1e-8)
        term = P * dp
        s2 = term.sum(2, keepdim=True)
        de = P * (dp - s2) * it
        # each term: C_DP U (P |dattn| + P |dlogprob| / (P + eps)); s2: their sum plus the sum's depth; de: the subtraction and
        # product (2 U of P(|dp| + |s2|)), * inv_temp (2 U |de|, 1/temp included)
        A_ = P * da.abs() + P * dl.abs() / (P + 1e-8)
        ds2 = (C_DP * U * A_).sum(2, keepdim=True) + depth * U * A_.sum(2, keepdim=True)
        err = (C_DP * U * A_ + P * ds2 + 2 * U * (A_ + P * s2.abs())) * it + 2 * U * de.abs()
    else:
        Pp = torch.where(valid, p_save.double(), z)
        P = torch.where(valid, P, z)
        s1 = (P * da).sum(2, keepdim=True)
        du = P * (da - s1) + dl
        x = du / (Pp + 1e-20)
        s2 = (Pp * x).sum(2, keepdim=True)
        de = Pp * (x - s2) * it
        ds1 = (depth + 1) * U * (P * da.abs()).sum(2, keepdim=True)
        du_abs = P * (da.abs() + s1.abs()) + dl.abs()
        ddu = P * ds1 + C_DU * U * du_abs
        rho = Pp / (Pp + 1e-20)
        dtau = rho * ddu + C_X * U * rho * du_abs
        ds2 = dtau.sum(2, keepdim=True) + depth * U * (rho * du_abs).sum(2, keepdim=True)
        err = (dtau + Pp * ds2 + U * (rho * du_abs + Pp * s2.abs())) * it + 2 * U * de.abs()
    return torch.where(valid, de, z), torch.where(valid, err, z)


def attention_grads(Q, K, v, in_lens, de, bounds=True):
    """float64 dQ [T,B,A], dK [L,B,A], dv [A] from a GIVEN de [B,T,L] (the kernel's de_work: exact fp32 values), chunked over T, and
    their bounds.  Per element (t, l, a), w = r (1 - r) = (1 - tanh^2)/4 and its error |dw| <= |1 - 2r| |dr| + U w + dr^2
    (fma(-r, r, r)).  The kernel's sums (attention.hip attn_dqdk_k):
      dQ[t,a] = 4 v sum_l de w      one thread, sequential over the len keys:                depth len + 2 (and * 4v)
      dK[l,a] = 4 v sum_t de w      a 32-row tile in 16 packed steps + pair add (sum form: 32 FMAs), then one fp32 atomic per
                                    tile in an unspecified order:                            depth 32 + 2 + ceil(T/32)
      dv[a]  = sum de (1 - 2r)      per key sum d - 2 sum d r (18), len keys per thread (32 len in the sum form), then one
                                    atomic per (b, tile):                                    depth 18 + len (or 32 len) + B ceil(T/32)
    The sums' bounds are depth U sum |terms| (terms: |de| w, resp. |de| (1 + 2r) for dv, where the kernel forms sum d - 2 sum dr)."""
    dev = de.device
    Qd, Kd, vd = Q.double().to(dev), K.double().to(dev), v.double().reshape(-1).to(dev)
    T, B, A = Qd.shape
    Lk = Kd.shape[0]
    lens = in_lens.to(dev).long().clamp(max=Lk)
    valid = torch.arange(Lk, device=dev)[None, :] < lens[:, None]
    Kd = torch.where(valid.t()[..., None], Kd, torch.zeros((), dtype=torch.float64, device=dev))
    Qb, Kb = Qd.transpose(0, 1), Kd.transpose(0, 1)
    D = torch.where(valid[:, None, :], de.double(), torch.zeros((), dtype=torch.float64, device=dev))   # [B,T,L]
    dQ = torch.zeros(B, T, A, dtype=torch.float64, device=dev)
    dK = torch.zeros(B, Lk, A, dtype=torch.float64, device=dev)
    dv = torch.zeros(A, dtype=torch.float64, device=dev)
    if bounds:
        eQ, sQ = torch.zeros_like(dQ), torch.zeros_like(dQ)
        eK, sK = torch.zeros_like(dK), torch.zeros_like(dK)
        eV, sV = torch.zeros(B, A, dtype=torch.float64, device=dev), torch.zeros(B, A, dtype=torch.float64, device=dev)
        qa, ka = Qb.abs(), Kb.abs()
    tc = _chunk_rows(B, Lk, A, dev)
    for t0 in range(0, T, tc):
        Dc = D[:, t0:t0 + tc]                                                         # [B,tc,L]
        x = Qb[:, t0:t0 + tc, None, :] + Kb[:, None, :, :]
        th = torch.tanh(x)
        g = Dc[..., None] * (4.0 * torch.sigmoid(2.0 * x) * torch.sigmoid(-2.0 * x))   # 1 - tanh^2 without cancellation at |x| > 19
        dQ[:, t0:t0 + tc] = g.sum(2)
        dK += g.sum(1)
        dv += torch.einsum("btl,btla->a", Dc, th)
        del th, g
        if bounds:
            r, s, dr = _r_and_err(x, qa[:, t0:t0 + tc, None, :] + ka[:, None, :, :])
            del x
            w = r * s
            dw = (r - s).abs() * dr + U * w + dr * dr
            Da = Dc.abs()[..., None]
            eQ[:, t0:t0 + tc] = (Da * dw).sum(2)
            sQ[:, t0:t0 + tc] = (Da * w).sum(2)
            eK += (Da * dw).sum(1)
            sK += (Da * w).sum(1)
            eV += (Da * 2.0 * dr).sum((1, 2))
            sV += (Da * (1.0 + 2.0 * r)).sum((1, 2))
            del r, s, dr, w, dw
    dQ = dQ * vd
    dK = dK * vd
    out = dict(dQ=dQ.transpose(0, 1), dK=dK.transpose(0, 1), dv=dv)
    if bounds:
        nT = -(-T // TT)
        big = sum_form_rows(Q).any(0) | sum_form_keys(K.to(dev), lens).any(0)               # [B]
        va4 = 4.0 * vd.abs()
        n_q = (lens.double() + 2.0)[:, None, None]
        out["dQ_err"] = (va4 * (eQ + n_q * U * sQ)).transpose(0, 1) + U * out["dQ"].abs()
        out["dK_err"] = (va4 * (eK + (34.0 + nT) * U * sK)).transpose(0, 1) + U * out["dK"].abs()
        n_v = 18.0 + lens.double() * torch.where(big, 32.0, 1.0) + B * nT
        out["dv_err"] = eV.sum(0) + (n_v[:, None] * U * sV).sum(0)
    return out


# ------------------------------------------------------------------------------------------------------------------ CTC
def ctc_ref(lp, in_lens, out_lens, blank=-1.0, gout=1.0, n_mean=None, bounds=True):
    """float64 attention-CTC of N samples: lp [N,T,L] in natural time, lengths [N].  loss = sum_b nll_b / K_b / n_mean over the
    feasible samples (zero_infinity), n_mean = N by default (the batch mean; the multi-flow call divides by F B).
    Returns dict(loss, nll [N], grad [N,T,L] of gout * loss, alpha / beta [N,T,2L+1], lse [N,T]) and, with bounds=True,
    the error bounds nll_err, loss_err and grad_err (see ctc_bounds).  Padding (t >= T_b, k >= K_b) is never read."""
    dev = lp.device
    N, T, L = lp.shape
    S = 2 * L + 1
    K = in_lens.to(dev).long().clamp(max=L)
    Tb = out_lens.to(dev).long().clamp(max=T)
    n_mean = N if n_mean is None else n_mean
    ninf = torch.tensor(-math.inf, dtype=torch.float64, device=dev)
    tt = torch.arange(T, device=dev)
    vk = torch.arange(L, device=dev)[None, :] < K[:, None]                                  # [N,L]
    vt = tt[None, :] < Tb[:, None]                                                          # [N,T]
    x = torch.where(vk[:, None, :] & vt[:, :, None], lp.double(), ninf)
    bl = torch.full((N, T, 1), float(blank), dtype=torch.float64, device=dev)
    full = torch.cat([bl, x], 2)
    lse = torch.logsumexp(full, 2)
    lse = torch.where(vt, lse, torch.zeros((), dtype=torch.float64, device=dev))
    # emission of each extended state, log-softmax normalised: even s blank, odd s = 2k+1 label k
    em = torch.full((N, T, S), -math.inf, dtype=torch.float64, device=dev)
    em[:, :, 0::2] = float(blank)
    em[:, :, 1::2] = x
    em = em - lse[..., None]
    sv = torch.arange(S, device=dev)[None, :] < (2 * K + 1)[:, None]                       # [N,S]
    em = torch.where(sv[:, None, :] & vt[:, :, None], em, ninf)
    skip = torch.zeros(S, dtype=torch.bool, device=dev)
    skip[3::2] = True
    alpha = torch.full((N, T, S), -math.inf, dtype=torch.float64, device=dev)
    beta = torch.full_like(alpha, -math.inf)
    z = torch.zeros((), dtype=torch.float64, device=dev)
    if bounds:
        Ea, Eb = torch.zeros_like(alpha), torch.zeros_like(alpha)
    a0 = em[:, 0].clone()
    a0[:, 2:] = -math.inf
    alpha[:, 0] = a0
    for t in range(1, T):
        pv = alpha[:, t - 1]
        p1 = torch.cat([ninf.expand(N, 1), pv[:, :-1]], 1)
        p2 = torch.where(skip, torch.cat([ninf.expand(N, 2), pv[:, :-2]], 1), ninf)
        l3 = torch.logsumexp(torch.stack([pv, p1, p2]), 0)
        a = l3 + em[:, t]
        alpha[:, t] = torch.where(vt[:, t, None], a, ninf)
        if bounds:
            ev = Ea[:, t - 1]
            e1 = torch.cat([z.expand(N, 1), ev[:, :-1]], 1)
            e2 = torch.cat([z.expand(N, 2), ev[:, :-2]], 1)
            fin = lambda y: torch.isfinite(y)                                               # noqa: E731
            m = torch.maximum(torch.where(fin(pv), ev, z), torch.where(fin(p1), e1, z))
            m = torch.maximum(m, torch.where(fin(p2), e2, z))
            logit = em[:, t] + lse[:, t, None]
            rho = U * (C_LSE3 + l3.abs() + (l3 + logit).abs() + a.abs())
            Ea[:, t] = torch.where(torch.isfinite(a) & vt[:, t, None], m + rho, z)
    for t in range(T - 1, -1, -1):
        init = em[:, t].clone()
        init = torch.where(torch.arange(S, device=dev)[None, :] >= (2 * K - 1)[:, None], init, ninf)
        if t + 1 < T:
            nx = beta[:, t + 1]
            n1 = torch.cat([nx[:, 1:], ninf.expand(N, 1)], 1)
            n2 = torch.cat([nx[:, 2:], ninf.expand(N, 2)], 1)
            n2 = torch.where(torch.roll(skip, -2) & (torch.arange(S, device=dev) % 2 == 1), n2, ninf)
            n3 = torch.logsumexp(torch.stack([nx, n1, n2]), 0)
            rec = n3 + em[:, t]
        else:
            rec = torch.full_like(init, -math.inf)
            n3 = rec
        last = (t == Tb - 1)[:, None]
        inner = (t < Tb - 1)[:, None]
        beta[:, t] = torch.where(last, init, torch.where(inner, rec, ninf))
        if bounds and t + 1 < T:
            ev = Eb[:, t + 1]
            e1 = torch.cat([ev[:, 1:], z.expand(N, 1)], 1)
            e2 = torch.cat([ev[:, 2:], z.expand(N, 2)], 1)
            m = torch.maximum(torch.where(torch.isfinite(nx), ev, z), torch.where(torch.isfinite(n1), e1, z))
            m = torch.maximum(m, torch.where(torch.isfinite(n2), e2, z))
            logit = em[:, t] + lse[:, t, None]
            rho = U * (C_LSE3 + n3.abs() + (n3 + logit).abs() + rec.abs())
            Eb[:, t] = torch.where(inner & torch.isfinite(rec), m + rho, z)
    idx = torch.arange(N, device=dev)
    tl = (Tb - 1).clamp(min=0)
    aT = alpha[idx, tl]                                                                    # [N,S]
    sl = 2 * K
    nll = -torch.logaddexp(aT[idx, sl], aT[idx, sl - 1])
    feas = torch.isfinite(nll) & (K > 0) & (Tb > 0)
    nll = torch.where(feas, nll, torch.full_like(nll, math.inf))
    per = torch.where(feas, nll / K.double() / n_mean, z)
    loss = per.sum()
    # gradient: (softmax_k - gamma_k) * gout / (K n_mean), gamma = exp(alpha + beta - em + nll) at the label states
    logp = x - lse[..., None]
    al, be, eml = alpha[:, :, 1::2], beta[:, :, 1::2], em[:, :, 1::2]
    gam = torch.exp(al + be - eml + nll[:, None, None])
    live = vk[:, None, :] & vt[:, :, None] & feas[:, None, None]
    scale = (gout / K.double().clamp(min=1) / n_mean)[:, None, None]
    sm = torch.exp(logp)
    grad = torch.where(live, (sm - gam) * scale, z)
    out = dict(loss=loss, nll=nll, grad=grad, alpha=alpha, beta=beta, lse=lse, feasible=feas, K=K, Tb=Tb, n_mean=n_mean)
    if bounds:
        out.update(ctc_bounds(x, lse, alpha, beta, Ea, Eb, nll, feas, K, Tb, vt, vk, live, blank, scale, sm, gam, grad, per, n_mean))
    return out


def ctc_bounds(x, lse, alpha, beta, Ea, Eb, nll, feas, K, Tb, vt, vk, live, blank, scale, sm, gam, grad, per, n_mean):
    """Bounds of the kernel's CTC (ctc.hip), from the float64 tables of the same inputs.
      lse_t (ctc_lse_k): m = max, s = expf(blank - m) + sum_k expf(x_k - m) (64-lane sum), m + logf(s).  Each term's relative error
        (2 + |x_k - m|) U (expf's ulp, x_k - m rounded), the sum's depth U, logf's ulp 2 U |log s|, the add U |lse|:  dlse_t.
      alpha_t[s] = lse3(alpha_{t-1}[s - 0, 1, 2]) + logit - lse_t: lse3 is 1-Lipschitz in the max norm, so the error is the largest
        of its (finite) predecessors' errors plus the step's own rho = U (C_LSE3 + |lse3| + |lse3 + logit| + |alpha_t|) -- the
        fp32 roundings scale with the MAGNITUDE of the unnormalised log-space values (thousands at T 862) -- and minus lse_t's error.
        beta likewise from t + 1.  The tables Ea / Eb hold the rounding part only: the kernel's lse_t error d_t enters alpha_t as
        -sum_{t'<=t} d_t', beta_t as -sum_{t'>=t} d_t', -logp as +d_t and nll as +sum_{t'} d_t', so it cancels EXACTLY in the
        posterior's exponent alpha + beta - logp + nll; it is added back for nll (and the loss) and for the softmax term.
      nll_b = -lse2(alpha_{T-1}[2K], alpha_{T-1}[2K-1]): max error + U (C_LSE3 + |nll|), plus sum_t dlse_t.
      loss = sum_b nll_b / K_b / n as fp32 atomics in an unspecified order: sum of the terms' errors (each + 3 U for the two
        divisions) + (n + 1) U sum |terms|.
      grad = (expf(logp) - expf(X)) * gout / K / n, X = alpha + beta + nll - logp (three adds: 3 U (|alpha|+|beta|+|nll|+|logp|)),
        logp = x - lse rounded (U |logp|): |dgamma| <= gamma (expm1(dX) + 2 U), |dsm| <= sm (expm1(dlse + U |logp|) + 2 U),
        plus the subtraction (U (sm + gamma)) and the scale (3 U |grad|)."""
    dev = x.device
    z = torch.zeros((), dtype=torch.float64, device=dev)
    N, T, L = x.shape
    m = torch.maximum(x.amax(2), torch.tensor(float(blank), dtype=torch.float64, device=dev))
    d = (x - m[..., None])
    w = torch.where(torch.isfinite(d), torch.exp(d), z)
    wb = torch.exp(blank - m)
    s = w.sum(2) + wb
    depth = torch.tensor([_wsum_depth(int(k) + 1) for k in K.tolist()], dtype=torch.float64, device=dev)[:, None]
    rel = U * ((w * (2.0 + torch.where(torch.isfinite(d), d.abs(), z))).sum(2) + wb * (2.0 + (blank - m).abs())) / s + depth * U
    dlse = rel + 2 * U * torch.log(s).abs() + U * lse.abs() + U * m.abs()
    dlse = torch.where(vt, dlse, z)
    idx = torch.arange(N, device=dev)
    tl = (Tb - 1).clamp(min=0)
    sl = 2 * K
    EaT = Ea[idx, tl]
    e_nll_r = torch.maximum(EaT[idx, sl], EaT[idx, sl - 1]) + U * (C_LSE3 + nll.abs().nan_to_num(0.0, 0.0, 0.0))
    nll_err = torch.where(feas, e_nll_r + dlse.sum(1), z)
    term_err = nll_err / K.double().clamp(min=1) / n_mean + 3 * U * per.abs()
    loss_err = term_err.sum() + (N + 1) * U * per.abs().sum()
    logp = x - lse[..., None]
    al, be = alpha[:, :, 1::2], beta[:, :, 1::2]
    lpa = torch.where(live, logp.abs(), z)
    dX = (Ea[:, :, 1::2] + Eb[:, :, 1::2] + e_nll_r[:, None, None] + U * lpa
          + 3 * U * (torch.where(live & torch.isfinite(al + be), al.abs() + be.abs(), z) + nll.abs().nan_to_num(0.0, 0.0, 0.0)[:, None, None] + lpa))
    dgam = torch.where(gam > 0, gam * (torch.expm1(dX) + 2 * U), z)      # unreachable state: alpha or beta is -inf in both, gamma = 0
    dsm = sm * (torch.expm1(dlse[..., None] + U * lpa) + 2 * U)
    gerr = scale * (dsm + dgam + U * (sm + gam)) + 3 * U * grad.abs()
    return dict(nll_err=nll_err, loss_err=loss_err, grad_err=torch.where(live, gerr, z), dlse=dlse)


def mirror(lp, out_lens, flag=True):
    """[B,T,L]: row t of utterance b -> row T_b - 1 - t for t < T_b (rows past T_b stay where they are) -- the reversed-time storage
    of a back-step flow (flowtron.py:250-256, ctc.hip CtcSrc)"""
    if not flag:
        return lp
    B, T = lp.shape[:2]
    t = torch.arange(T, device=lp.device)[None, :]
    Tb = out_lens.to(lp.device).long().clamp(max=T)[:, None]
    src = torch.where(t < Tb, Tb - 1 - t, t)
    return lp.gather(1, src[..., None].expand_as(lp))


def ctc_multi_ref(lps, reversed_, in_lens, out_lens, blank=-1.0, gout=1.0, bounds=True):
    """The stacked F-flow call (ft_attn_ctc_*_multi): flow f's tensor is in reversed time when reversed_[f]; sample f B + b; the loss
    divides by F B.  Returns the ctc_ref dict of the stacked natural-time samples plus `grads`: the per-flow gradients mirrored back
    into each flow's own time order (and `grad_errs` likewise)."""
    F_ = len(lps)
    B = lps[0].shape[0]
    nat = torch.cat([mirror(lp, out_lens, bool(r)) for lp, r in zip(lps, reversed_)], 0)
    r = ctc_ref(nat, in_lens.repeat(F_), out_lens.repeat(F_), blank, gout, n_mean=F_ * B, bounds=bounds)
    r["grads"] = [mirror(r["grad"][f * B:(f + 1) * B], out_lens, bool(reversed_[f])) for f in range(F_)]
    if bounds:
        r["grad_errs"] = [mirror(r["grad_err"][f * B:(f + 1) * B], out_lens, bool(reversed_[f])) for f in range(F_)]
    return r
