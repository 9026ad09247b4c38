"""Float64 replay of the teacher-forced cumulative attention (ft_cumm_attn_fwd / _bwd: csrc/cumm_fused.hip, csrc/cumm_attn.hip), ONE
FRAME AT A TIME, with the kernels' operand rounding and a propagated per-element error bound (imported by the tests, not collected).
Plain torch on whatever device the operands live on; nothing here calls the project's kernels or the oracle.

Every frame starts from the KERNEL'S OWN saved state -- attn[:, i-1], cumm_all[i] and kproj_all[i] (fused path: tanh(Q_i + K_i) on
the rows l < in_lens[b]; launch chain: K_i) -- so a deviation in one frame can neither hide behind nor be blamed on an earlier one.

Values travel as EV = (v, e): the float64 value and a bound on |kernel - v|, propagated BY THE SAME COMPUTATION ON ABSOLUTE VALUES
(running error analysis).  Nothing is stored, nothing is fitted to the kernel.  u = 2^-24:

  * an fp32 add / multiply / fma rounds once: u |result|; a sum of n terms in ANY order: n u sum |terms|;
  * MFMA chains (16-bit operands, products exact in fp32): n = ceil(K / 32) + 32 -- ASSUMPTION ABOUT THE HARDWARE, as gemm_ref64:
    every addition inside a matrix instruction rounds (or truncates) at most once to fp32 or better, in an order that is not
    assumed; a split of K over s slices adds s and removes at least as many chained instructions, so the count holds for any split.
    One exception was measured and is part of the assumption: a SUBNORMAL fp16 operand is weighed as the smallest normal (`lifted`);
    The library GEMMs (ft_gemm, ft_gemm_img) get the same count plus their epilogue, with gemm_ref64's truncation-proof 2 u;
  * sigmoid / tanh in the v_exp_f32 / v_rcp_f32 forms: ACT_EPS = 2^-20 absolute (the constant of test_gpu_recurrence_replay.py) on
    top of the argument's error times the slope (slope taken over the error interval: |sigmoid''| <= 0.1, |tanh''| <= 0.77);
  * expf / logf 3 ulp, division 2.5 ulp (OpenCL full profile, as elementwise_ref64), 1 ulp = 2 u;
  * an intermediate the kernel rounds to 16 bits RESETS the error: round(v - e) == round(v + e) means every value the kernel can
    hold rounds to the same 16-bit number (rounding is monotone) and the result is exact; only where the two differ -- the float64
    value lies within its own bound of a rounding boundary -- the element passes on the distance to the farther candidate (one
    16-bit ulp).  Which elements are ambiguous is decided from the reference alone.  A relu whose argument straddles zero likewise
    passes on |argument| + its bound, and its gate in the backward passes on the whole gated value;
  * the (dcumm, dprev) carry of the backward is fp32 and never reset: its bound is carried through the frame scan.

Rounding points found in the code (fmt 1 / 2; fmt 0 = the fp32 launch chain rounds nowhere; fmt None = unrounded float64):
  forward   col2 = op16(h1) (col_frags), op16(w2) and op16(W_key) (cvt16_frag_k), km = op16(text * cond) (pack4: the PRODUCT is
            rounded), ctx = op16(attn) . op16(V) (bgemm);
  backward  DV = op16(dctx) . op16(V), dV = op16(attn)^T . op16(dctx) (bgemm); dK16 = op16(s v (1 - t^2)) feeds dkm AND dW_key while
            dQ sums the UNROUNDED dK; op16(W_key^T), op16(w2^T); km and col2 recomputed and rounded as in the forward; dpre2 rounded
            (feeds dcol2, dw2 and -- through the column of ones of the col2 stream -- db2, which therefore sums the ROUNDED dpre2).
The saved tanh, the scores, attn, cumm, dtext, dv, dw1, db1 and the carry stay fp32.

`mut` names a deliberately WRONG reference (MUT_FWD / MUT_BWD) for the sharpness checks."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
ACT_EPS = 2.0 ** -20
EXP_ULP, LOG_ULP, DIV_ULP = 3.0, 3.0, 2.5
SECOND_ORDER = 1.0 + 2.0 ** -10          # first-order propagation through the softmax: products of two bounds are below 2^-10 of one
FLOOR = 2.0 ** -125                      # fp32 results below the normal range may be flushed
EPS_LP = float(torch.tensor(1e-8, dtype=torch.float32))
SHARP = 10.0
F64 = torch.float64
BWD_OWN, FWD_ROWS = 26, 32

MUT_FWD = ("prev_i2", "cumm_stale", "tap_shift", "h1_len", "w2_noround", "wk_noround", "text_round", "drop_kstep", "text_nb",
           "mask_le", "no_temp", "no_eps")
MUT_BWD = ("no_eps", "no_carry", "halo_zero", "top_chunk", "db2_one", "tap_shift", "no_temp")
OUT_BWD = ("dQ", "dV", "dtext", "dw_key", "dv", "dw1", "db1", "dw2", "db2")


def make_inputs(T, L, lens, E=640, A=640, seed=0, cls="aligned", w1_scale=0.3, device="cpu"):
    """fp32-valued float64 inputs and upstream gradients of one call.

    cls "signed": the scales of the op-level test of tests/test_gpu_ops.py (N(0, 1) data).  The forward's bounds are tight on it; the
    backward's are valid but wide: a worst-case bound passes through three reductions per frame whose terms cancel (sum |terms| /
    |sum| ~ sqrt(K) each), and the 16-bit roundings in between turn a wide bound into one 16-bit ulp for every element.
    cls "aligned": the condition on the inputs that keeps the backward's bound tight -- text, W_key, v, w1 and w2 non-negative, so
    that the terms of dkm = W_key^T dK, dcol2 = w2^T dpre2 and of the first convolution's adjoint share the sign of s_l and do not
    cancel; W_key sparse (16 of 640 per row) so that the keys still differ from position to position; b1 signed (relu gates of
    both kinds), b2 centred on the middle of the sigmoid.  In both classes V and dctx are dyadic (multiples of 1/8 and 1/64):
    dctx . V, the long reduction in FRONT of the softmax backward's cancellation, is then exact in any order (exact_any_order).
    w1_scale scales the first convolution and with it the (dcumm, dprev) carry: the long (chunked) cases use a small one, because the
    carry's bound is never reset and grows from frame to frame."""
    B = len(lens)
    gen = torch.Generator().manual_seed(1000 + 31 * T + L + seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    ri = lambda *s: torch.randint(-8, 9, s, generator=gen).double()
    if cls == "signed":
        d = dict(text=rn(L, B, E) * 0.7, Q=rn(T, B, A) * 0.7, V=ri(L, B, A) / 8, wk=rn(A, E) / E ** 0.5 * 1.5, v=rn(A) / A ** 0.5 * 6.0,
                 w1=rn(32, 2, 5) * 2 * w1_scale, b1=rn(32) * 0.3, w2=rn(E, 32, 3) * 0.25, b2=rn(E) * 0.3)
    else:
        keep = (torch.rand(A, E, generator=gen, dtype=F64) < 16.0 / E).double()
        d = dict(text=rn(L, B, E).abs() * 0.7, Q=rn(T, B, A) * 0.7, V=ri(L, B, A) / 8, wk=rn(A, E).abs() * 0.3 * keep,
                 v=rn(A).abs() / A ** 0.5 * 12.0, w1=rn(32, 2, 5).abs() * 2 * w1_scale, b1=rn(32) * 0.3, w2=rn(E, 32, 3).abs() * 0.25,
                 b2=rn(E) - 2.0)
    up = dict(dctx=ri(T, B, A) / 64, dattn=rn(B, T, L), dlp=rn(B, T, L) * 0.1)
    f32 = lambda t: t.float().double().to(device)
    return {k: f32(t) for k, t in d.items()}, {k: f32(t) for k, t in up.items()}


class EV:
    """value and bound; e None = exact"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v, self.e = v, e

    def err(self):
        return torch.zeros_like(self.v) if self.e is None else self.e

    def __getitem__(self, idx):
        return EV(self.v[idx], None if self.e is None else self.e[idx])


def _ev(x):
    if isinstance(x, EV):
        return x
    return EV(x if torch.is_tensor(x) else torch.tensor(float(x), dtype=F64))


def add(a, b, n=1):
    a, b = _ev(a), _ev(b)
    v = a.v + b.v
    return EV(v, a.err() + b.err() + n * U * v.abs() + FLOOR)


def mul(a, b, n=1):
    a, b = _ev(a), _ev(b)
    v = a.v * b.v
    e = n * U * v.abs() + FLOOR
    if a.e is not None:
        e = e + a.e * b.v.abs()
    if b.e is not None:
        e = e + b.e * a.v.abs()
    if a.e is not None and b.e is not None:
        e = e + a.e * b.e
    return EV(v, e)


SUB16 = 2.0 ** -14                       # smallest normal fp16


def lifted(x, fmt):
    """|x| as the fp16 matrix instruction weighs it when it aligns the products of one instruction: a SUBNORMAL fp16 operand carries the
    exponent field of the smallest normal, so the sum's rounding is relative to |x| lifted to 2^-14 (ASSUMPTION ABOUT THE HARDWARE,
    from a measurement: 2^-24 * 1.41210938 - 2^-24 * 0.0148849487 through ft_gemm in fp16 mode comes out as 183144 x 2^-41, a multiple
    of 2^-38, although either product alone and the same sum with both operands scaled by 1024 are exact -- 183137 x 2^-41)"""
    x = x.abs()
    if fmt != 2:
        return x
    return torch.where((x > 0) & (x < SUB16), torch.full_like(x, SUB16), x)


def lin(fn, a, w, n, k, sub=None):
    """a bilinear map fn(x, w) (matmul, convolution, einsum) of an EV and an EXACT operand, k products per output element summed in any
    order with n roundings; each product or partial sum below the normal range may be flushed (FLOOR each)"""
    e = n * U * fn(lifted(a.v, sub), lifted(w, sub)) + 2 * k * FLOOR
    if a.e is not None:
        e = e + fn(a.e, w.abs())
    return EV(fn(a.v, w), e)


def bil(fn, a, b, n, k, sub=None):
    """the same with two EV operands (sub: the operand format of a matrix-instruction reduction, see `lifted`)"""
    a, b = _ev(a), _ev(b)
    e = n * U * fn(lifted(a.v, sub), lifted(b.v, sub)) + 2 * k * FLOOR
    if a.e is not None:
        e = e + fn(a.e, b.v.abs())
    if b.e is not None:
        e = e + fn(a.v.abs(), b.e)
    if a.e is not None and b.e is not None:
        e = e + fn(a.e, b.e)
    return EV(fn(a.v, b.v), e)


def exact_any_order(a, w, abs_sum, bits=8):
    """gemm_ref64's exact class: both operands integer multiples of 2^-bits and every sum of |products| below 2^24 quanta of 2^-2 bits --
    every partial sum, in any order and any split, is then an fp32 number and the kernel's result carries no rounding at all"""
    q = 2.0 ** bits
    return bool((a * q == torch.round(a * q)).all() and (w * q == torch.round(w * q)).all() and float(abs_sum.max()) * q * q < 2.0 ** 24)


def rnd(v, fmt):
    """fp32 -> operand format -> back, round to nearest even (fmt 1 bf16, 2 fp16; 0 / None: as it is)"""
    if not fmt:
        return v
    return v.float().to(torch.bfloat16 if fmt == 1 else torch.float16).to(v.dtype)


def op16(x, fmt):
    x = _ev(x)
    if not fmt:
        return x
    r = rnd(x.v, fmt)
    if x.e is None:
        return EV(r)
    return EV(r, torch.maximum((rnd(x.v + x.e, fmt) - r).abs(), (rnd(x.v - x.e, fmt) - r).abs()))


def sigmoid(x):
    s = torch.sigmoid(x.v)
    e = x.err()
    return EV(s, (s * (1 - s) + 0.1 * e) * e + ACT_EPS)


def tanh(x):
    t = torch.tanh(x.v)
    e = x.err()
    return EV(t, ((1 - t * t) + 0.77 * e) * e + ACT_EPS)


def n_mfma(K):
    return math.ceil(K / 32) + 32


def n_lib(K, fmt):
    """ft_gemm / ft_gemm_img, any split: units of u (gemm_ref64's u is 2^-23).  fp32 mode: the products round too and nothing is assumed
    about the kernel's order -- a term passes through at most K additions, + product, bias and epilogue"""
    if fmt == 0:
        return K + 8
    return 2 * (n_mfma(K) + 4)


def conv(x, w, pad):
    """Conv1d with zero padding at the ends as im2col + einsum: x [B,C,L], w [O,C,K] -> [B,O,L] (float64 on any device)"""
    xu = F.pad(x, (pad, pad)).unfold(2, w.shape[2], 1)                                           # x[b][c][l + k - pad]
    return torch.einsum("bclk,ock->bol", xu, w)


def conv_t(y, w, pad):
    """its adjoint: dx[b][c][m] = sum_{o,k} w[o][c][k] y[b][o][m - k + pad]"""
    yu = F.pad(y, (pad, pad)).unfold(2, w.shape[2], 1)                                           # y[b][o][m + j - pad], j = K - 1 - k
    return torch.einsum("bomj,ocj->bcm", yu, w.flip(2))


class Params:
    """the fp32 inputs of a call as float64 tensors: text [L,B,E], Q [T,B,A], V [L,B,A], wk [A,E], v [A], w1 [NF,2,K1], b1, w2
    [E,NF,K2], b2, in_lens (list), temp"""

    def __init__(self, text, Q, V, wk, v, w1, b1, w2, b2, in_lens, temp):
        self.text, self.Q, self.V, self.wk, self.v, self.w1, self.b1, self.w2, self.b2 = (
            t.to(F64) for t in (text, Q, V, wk, v.reshape(-1), w1, b1, w2, b2))
        self.T, self.B, self.A = Q.shape
        self.L, _, self.E = text.shape
        self.NF, _, self.K1 = w1.shape
        self.K2 = w2.shape[2]
        self.lens = [min(int(x), self.L) for x in in_lens]
        self.temp = float(torch.tensor(float(temp), dtype=torch.float32))          # the fp32 argument of the call
        ar = torch.arange(self.L, device=text.device)
        self.valid = ar[None, :] < torch.tensor(self.lens, device=text.device)[:, None]              # [B, L]

    def mask(self, mut):
        if mut != "mask_le":
            return self.valid
        ar = torch.arange(self.L, device=self.text.device)
        return ar[None, :] <= torch.tensor(self.lens, device=self.text.device)[:, None]


class State:
    """what the kernel saved: attn [B,T,L], cumm_all [T,B,L], kproj [T,L,B,A] (tanh on the valid rows / K_i), as float64"""

    def __init__(self, attn, cumm_all, kproj, P):
        self.attn, self.cumm = attn.to(F64), cumm_all.to(F64)
        self.kproj = kproj.to(F64).reshape(P.T, P.L, P.B, P.A)


def cumm_exact(st, i):
    """the fp32 running sum cumm_all[i-1] + attn[:, i-1] (both kernels: one fp32 addition per element), frame 0: zeros"""
    if i == 0:
        return torch.zeros_like(st.cumm[0])
    return (st.cumm[i - 1].float() + st.attn[:, i - 1].float()).double()


def cond_chain(P, st, i, fmt, mut=None):
    """location features of frame i from the saved state: pre1, h1, col2 (all [B,NF,L]), cond and km ([L,B,E]), x [B,2,L]"""
    zeros = torch.zeros_like(st.cumm[0])
    cumm = st.cumm[i]
    prev = st.attn[:, i - 1] if i > 0 else zeros
    if mut == "prev_i2":
        prev = st.attn[:, i - 2] if i > 1 else zeros
    if mut == "cumm_stale":
        cumm = st.cumm[i - 1] if i > 0 else zeros
    x = torch.stack([cumm, prev], 1)
    xin = torch.roll(x, 1, 2) if mut == "tap_shift" else x
    pad1, pad2 = P.K1 // 2, P.K2 // 2
    n1 = 2 * P.K1 + 1 if fmt != 0 else n_lib(2 * P.K1, 0)
    v = conv(xin, P.w1, pad1) + P.b1[None, :, None]
    pre1 = EV(v, n1 * U * (conv(xin.abs(), P.w1.abs(), pad1) + P.b1.abs()[None, :, None]))
    h1 = EV(torch.relu(pre1.v), torch.where(pre1.v + pre1.e > 0, pre1.e, torch.zeros_like(pre1.e)))
    if mut == "h1_len":
        h1 = EV(h1.v * P.valid[:, None, :], h1.e * P.valid[:, None, :])
    col2 = op16(h1, fmt)
    w2r = P.w2 if mut == "w2_noround" else rnd(P.w2, fmt)
    n2 = n_mfma(P.NF * P.K2) if fmt != 0 else n_lib(P.NF * P.K2, 0)
    pre2 = lin(lambda a, w: conv(a, w, pad2), col2, w2r, n2, P.NF * P.K2, fmt)
    pre2 = add(pre2, P.b2[None, :, None])
    cond = sigmoid(pre2)
    cond = EV(cond.v.permute(2, 0, 1), cond.e.permute(2, 0, 1))                                   # [L, B, E]
    text = torch.roll(P.text, 1, 1) if mut == "text_nb" else P.text
    if mut == "text_round":
        km = mul(rnd(text, fmt), cond)
    else:
        km = op16(mul(text, cond), fmt)
    return dict(x=x, xin=xin, pre1=pre1, h1=h1, col2=col2, cond=cond, km=km, w2r=w2r, text=text)


def softmax_ev(e, mask, L):
    """softmax over the masked positions of e [B, L] (EV): relative error of p_l <= its own exponent's error + the p-weighted mean of
    all of them + the sum's and the division's roundings"""
    ninf = torch.full_like(e.v, -math.inf)
    ev_ = torch.where(mask, e.v, ninf)
    m = ev_.max(1, keepdim=True).values
    d = torch.where(mask, ev_ - m, torch.zeros_like(ev_))
    p = torch.softmax(ev_, 1)
    rel = torch.where(mask, e.err() + U * d.abs() + 2 * EXP_ULP * U, torch.zeros_like(d))
    agg = (p * rel).sum(1, keepdim=True)
    n_s = math.ceil(L / 256) + 8
    return EV(p, p * (rel + agg + (n_s + 2 * DIV_ULP) * U) * SECOND_ORDER + FLOOR * mask)


def frame_fwd(P, st, i, fmt, mut=None):
    """frame i: EVs of the saved tensor (tanh or K), attn_i, logprob_i, and the bit-exact running sum"""
    fused = fmt != 0
    c = cond_chain(P, st, i, fmt, mut)
    wkr = P.wk if mut == "wk_noround" else rnd(P.wk, fmt)
    km = c["km"]
    if mut == "drop_kstep":
        km = EV(km.v.clone(), km.e)
        km.v[..., 32:64] = 0
    K = lin(lambda a, w: a @ w.t(), km, wkr, n_mfma(P.E) if fused else n_lib(P.E, 0), P.E, fmt)
    q = P.Q[i][None]
    if fused:
        saved = tanh(add(K, q))
        vl = P.valid.t()[:, :, None]
        t = EV(torch.where(vl, st.kproj[i], torch.zeros_like(st.kproj[i])))      # downstream of the check: the kernel's own tanh
        n_e = 32
        e = lin(lambda a, w: a @ w, t, P.v, n_e, P.A)              # [L, B]
    else:
        saved = K
        t = tanh(add(EV(st.kproj[i]), q))
        # (sum v - 2 sum v r) / temperature, r = (1 - t) / 2: the two sums' roundings on 3 sum |v|
        e = lin(lambda a, w: a @ w, t, P.v, 0, P.A)
        e = EV(e.v, e.err() + (math.ceil(P.A / 64) + 10) * U * 3 * P.v.abs().sum())
    sc = 1.0 if mut == "no_temp" else 1.0 / P.temp
    e = EV(e.v.t() * sc, e.err().t() * sc + 2 * U * (e.v.t() * sc).abs())
    mask = P.mask(mut)
    p = softmax_ev(e, mask, P.L)
    a_k = st.attn[:, i]                                       # logprob from the kernel's own attention
    lp_v = torch.log(a_k + (0.0 if mut == "no_eps" else EPS_LP)).clamp_min(-1e30)
    lp = EV(lp_v, U + 2 * LOG_ULP * U * lp_v.abs())
    return dict(saved=saved, attn=p, logprob=lp, mask=mask)


def ctx_ref(P, st, fmt):
    """ctx [T,B,A] = attn . V over all frames: the batched GEMM (operands rounded) / the chain's fp32 fma loop"""
    a, V = rnd(st.attn, fmt), rnd(P.V, fmt)
    n = n_lib(P.L, fmt) if fmt != 0 else math.ceil(P.L / 4) + 4
    return lin(lambda x, w: torch.einsum("btl,lba->tba", x, w), EV(a), V, n, P.L, fmt)


def simulate_fwd(P, fmt):
    """a free-running forward of the replay itself (CPU tests: stands in for the kernel's saved state); fp32-valued like the kernel's"""
    f32 = lambda t: t.float().double()
    dev = P.text.device
    st = State(torch.zeros(P.B, P.T, P.L, dtype=F64, device=dev), torch.zeros(P.T, P.B, P.L, dtype=F64, device=dev),
               torch.zeros(P.T, P.L, P.B, P.A, dtype=F64, device=dev), P)
    for i in range(P.T):
        st.cumm[i] = cumm_exact(st, i)
        c = cond_chain(P, st, i, fmt)
        K = c["km"].v @ rnd(P.wk, fmt).t()
        t = torch.tanh(K + P.Q[i][None])
        st.kproj[i] = f32(t) if fmt != 0 else f32(K)
        e = (f32(t) @ P.v).t() / P.temp
        e = torch.where(P.valid, e, torch.full_like(e, -math.inf))
        st.attn[:, i] = f32(torch.softmax(e, 1))
    return st


# ------------------------------------------------------------------------------------------------------------------ backward
def replay_bwd(P, st, dctx, dattn, dlp, fmt, chunk=None, mut=None):
    """all nine gradients as EVs, from the kernel's saved forward and the upstream gradients (dattn / dlp may be None)"""
    fused = fmt != 0
    T, B, L, A, E, NF, K1, K2 = P.T, P.B, P.L, P.A, P.E, P.NF, P.K1, P.K2
    dctx = dctx.to(F64)
    dev = dctx.device
    valid = P.mask(mut)
    vl = valid.t()[:, :, None]                                                                   # [L, B, 1]
    nwg = B * math.ceil(L / BWD_OWN)
    R = L * B
    d16, V16, a16 = rnd(dctx, fmt), rnd(P.V, fmt), rnd(st.attn, fmt)
    DV = lin(lambda x, w: torch.einsum("tba,lba->btl", x, w), EV(d16), V16, n_lib(A, fmt) if fused else math.ceil(A / 64) + 8, A, fmt)
    if exact_any_order(d16, V16, torch.einsum("tba,lba->btl", d16.abs(), V16.abs())):
        DV = EV(DV.v, torch.zeros_like(DV.v))            # (the tight cases feed dyadic dctx and V: dctx . V is then exact in any order)
    dV = lin(lambda x, w: torch.einsum("btl,tba->lba", x, w), EV(a16), d16, n_lib(T, fmt) if fused else T + 1, T, fmt)
    wkr = rnd(P.wk, fmt)
    # counts of the accumulated outputs (any order)
    n_dq = (math.ceil(L / BWD_OWN) + 9) if fused else math.ceil(L / 4) + 4
    n_dv = (T + math.ceil(nwg / 4) + 12) if fused else math.ceil(L / 4) + 5 + T * B
    if fused:
        Tc = min(chunk or T, T)
        n_wg = 2 * (math.ceil(Tc * R / 32) + 33 + math.ceil(T / Tc) + 4)
        n_w1 = BWD_OWN + T + math.ceil(nwg / 4) + 5
    else:
        n_wg = n_w1 = R + 16 + T
    zeroBL = torch.zeros(B, L, dtype=F64, device=dev)
    g_prev, g_cumm = EV(zeroBL, zeroBL.clone()), EV(zeroBL, zeroBL.clone())
    out = {k: None for k in OUT_BWD}
    dQ_v, dQ_e = torch.zeros(T, B, A, dtype=F64, device=dev), torch.zeros(T, B, A, dtype=F64, device=dev)

    def acc(name, x):
        out[name] = x if out[name] is None else EV(out[name].v + x.v, out[name].err() + x.err())

    sc = 1.0 if mut == "no_temp" else 1.0 / P.temp          # (the fp32 reciprocal's rounding is counted with the multiplication: n = 2)
    for i in range(T - 1, -1, -1):
        p = st.attn[:, i]
        if mut == "no_carry":
            g_prev, g_cumm = EV(zeroBL, zeroBL.clone()), EV(zeroBL, zeroBL.clone())
        d = add(add(DV[:, i], g_prev), g_cumm)
        if dattn is not None:
            d = add(d, dattn[:, i].to(F64))
        if dlp is not None:
            den = p + (0.0 if mut == "no_eps" else EPS_LP)
            term = torch.where(valid, dlp[:, i].to(F64) / den.clamp_min(1e-30), zeroBL)
            d = add(d, EV(term, (2 * DIV_ULP + 2) * U * term.abs()))
        d = EV(d.v * valid, d.e * valid)
        sm = bil(lambda a_, b_: (a_ * b_).sum(1, keepdim=True), EV(p), d, math.ceil(L / 256) + 9, L)
        s = mul(mul(EV(p), add(d, EV(-sm.v, sm.e))), sc, 2)                                     # [B, L]
        s = EV(s.v * valid, s.e * valid)
        if fused:
            t = EV(torch.where(vl, st.kproj[i], torch.zeros_like(st.kproj[i])))      # (rows beyond in_len are not the kernel's)
            g1 = EV(1 - t.v * t.v, U * (1 - t.v * t.v).abs())
        else:
            t = tanh(add(EV(st.kproj[i]), P.Q[i][None]))
            g1 = EV(1 - t.v * t.v, 2 * t.v.abs() * t.e + t.e * t.e + 3 * U)
        s_lb = EV(s.v.t()[:, :, None], s.e.t()[:, :, None])
        dK = mul(mul(s_lb, P.v), g1)                                                             # [L, B, A]
        dq = EV(dK.v.sum(0), dK.e.sum(0) + n_dq * U * dK.v.abs().sum(0) + L * FLOOR)
        dQ_v[i], dQ_e[i] = dq.v, dq.e
        acc("dv", bil(lambda a_, b_: (a_ * b_).sum((0, 1)), s_lb, t, n_dv, R))
        dK16 = op16(dK, fmt)
        c = cond_chain(P, st, i, fmt, mut)
        cond, km, text = c["cond"], c["km"], c["text"]
        n_k = n_mfma(A) if fused else n_lib(A, 0)

        def tail(dK16_):
            dkm = lin(lambda a_, w: a_ @ w, dK16_, wkr, n_k, A, fmt)                                    # [L, B, E]
            dp2 = mul(mul(mul(dkm, text), cond), add(EV(-cond.v, cond.e), 1.0))
            dp2 = op16(dp2, fmt)
            dp2c = EV(dp2.v.permute(1, 2, 0), dp2.err().permute(1, 2, 0))                       # [B, E, L]
            n_c = (math.ceil(E / 128) + 32 + 12) if fused else n_lib(E, 0) + K2
            dh1 = lin(lambda a_, w: conv_t(a_, w, K2 // 2), dp2c, c["w2r"], n_c, E * K2, fmt)
            pre1 = c["pre1"]
            on = (pre1.v > 0) & ~((mut == "h1_len") & ~valid[:, None, :])
            amb = pre1.v.abs() <= pre1.e
            dpre1 = EV(dh1.v * on, torch.where(amb, dh1.v.abs() + dh1.e, dh1.e * on))
            n_s2 = (NF * K1 // 4 + 2 + 1) if fused else n_lib(NF, 0) + K1
            ds2 = lin(lambda a_, w: conv_t(a_, w, K1 // 2), dpre1, P.w1, n_s2, NF * K1)
            return dkm, dp2, dpre1, ds2

        dkm, dp2, dpre1, ds2 = tail(dK16)
        if mut == "halo_zero" and L > BWD_OWN:
            # the tile that owns rows 26 .. 51 with its lower halo rows (23 .. 25) of dK zeroed: dcol2 of row 25 is missing from its
            # dh1 at row 26, so dpre1 (dw1, db1) and the carry are wrong on its first own rows
            cut = EV(dK16.v.clone(), dK16.err().clone())
            cut.v[:BWD_OWN], cut.e[:BWD_OWN] = 0, 0
            _, _, dpre1b, ds2b = tail(cut)
            splice = lambda x, y: EV(torch.cat([x.v[..., :BWD_OWN], y.v[..., BWD_OWN:]], -1), torch.cat([x.e[..., :BWD_OWN], y.e[..., BWD_OWN:]], -1))
            dpre1, ds2 = splice(dpre1, dpre1b), splice(ds2, ds2b)
        acc("dtext", mul(dkm, cond, T + 1))
        rows = lambda x: x.reshape(R, -1)
        top = mut == "top_chunk" and chunk and i >= (T - 1) // chunk * chunk and (T - 1) // chunk > 0
        if not top:
            acc("dw_key", bil(lambda a_, b_: a_.t() @ b_, EV(rows(dK16.v), rows(dK16.err())), EV(rows(km.v * vl), rows(km.err() * vl)), n_wg, T * R, fmt))
            col2 = c["col2"]
            pad = K2 // 2
            unf = lambda x: F.pad(x.permute(1, 2, 0), (pad, pad)).unfold(2, K2, 1).permute(2, 0, 1, 3).reshape(R, NF * K2)
            # col2 rows of the VALID positions: taps reach h1 at l +- 1 whatever its validity
            cfull = EV(col2.v.permute(2, 0, 1), col2.err().permute(2, 0, 1))
            cu = EV(unf(cfull.v) * rows(vl.double()), unf(cfull.err()) * rows(vl.double()))
            acc("dw2", bil(lambda a_, b_: a_.t() @ b_, EV(rows(dp2.v), rows(dp2.err())), cu, n_wg, T * R, fmt))
        if not (mut == "db2_one" and i == 0) and not top:
            acc("db2", EV(dp2.v.sum((0, 1)), dp2.err().sum((0, 1)) + n_wg * U * lifted(dp2.v, fmt).sum((0, 1)) + T * R * FLOOR))
        xin = c["xin"]
        xu = F.pad(xin, (K1 // 2, K1 // 2)).unfold(2, K1, 1)                                     # [B, 2, L, K1]: x[ch][l + k - 2]
        acc("dw1", lin(lambda a_, w: torch.einsum("bcl,bhlk->chk", a_, w), dpre1, xu, n_w1, T * R))
        acc("db1", EV(dpre1.v.sum((0, 2)), dpre1.e.sum((0, 2)) + n_w1 * U * dpre1.v.abs().sum((0, 2)) + T * R * FLOOR))
        g_prev = EV(ds2.v[:, 1] * valid, ds2.e[:, 1] * valid)
        gc = add(g_cumm, EV(ds2.v[:, 0], ds2.e[:, 0]))
        g_cumm = EV(gc.v * valid, gc.e * valid)
    out["dQ"] = EV(dQ_v, dQ_e)
    out["dV"] = dV
    out["dw2"] = EV(out["dw2"].v.reshape(E, NF, K2), out["dw2"].err().reshape(E, NF, K2))
    out["carry"] = (g_prev, g_cumm)
    return out
