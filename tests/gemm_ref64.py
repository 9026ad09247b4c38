"""Float64 restatement of the GEMM entry points (ft_gemm, ft_gemm_img, ft_img_gemv_rows / _bwd), two input classes, a per-element
error bound and the wrong references of the sensitivity checks (imported by the tests, not collected).  Plain torch, on whatever
device the operands live on; nothing here calls the project's kernels.

The formula (include/flowtron_hip.h), operands first rounded to the operand format (bf16 / fp16 round-to-nearest-even; FT_F32: as
they are):

    C[row][n] = act( alpha * sum_k a[m][k] b[n][k] + beta * C0[row][n] + bias[n] + r1_row[row] * r1_col[n] )

row = the OUTPUT row (after the row map); the rank-1 term is not scaled by alpha; FT_GEMM_C16 rounds the result once to the operand
format.  Compact rows, k_shift, a_rows and pointers inside an image are restated as plain indexing on the fp32 sources (`operands`).

Input class "exact": operands integers in [-8, 8], alpha / beta signed powers of two, C0 / bias / rank-1 vectors small integers,
activation none or relu.  Every partial sum, in ANY order and any split, is then an integer multiple of the smallest power of two in
play and below 2^24 of them (`exact_case` asserts it), so fp32 arithmetic commits no rounding at all and a correct kernel equals the
reference BIT FOR BIT -- on the atomic split-K paths too.  With C16, "equal" is the one RNE rounding of that exact value.  This is
the class that carries the long reductions: at K = 8192 a random-data tolerance is as large as one missing product.

Input class "rounded": N(0, 1) data, alpha = 1 / sqrt(K), with exact ties of both 16-bit formats, fp16 subnormals and values at the
fp16 overflow edge planted (and, for the staging path that rounds in the kernel, exact zeros).  Compared under the bound.

The bound, per element, u = 2^-23 (so a truncating accumulator passes too):

    u * [ (n_instr + P + slices) * |alpha| sum_k |a b|  +  c * (|alpha dot| + |beta C0| + |bias| + |r1|) ]   (+ activation, + C16)

  * n_instr = matrix instructions chained on one accumulator in one k-slice (ceil(K_slice / P)); P = products per instruction
    (32 for the 16-bit MFMA 16x16x32, 4 for the fp32 16x16x4): a term passes through at most P additions inside its instruction and
    n_instr accumulator additions.  ASSUMPTION ABOUT THE HARDWARE: each addition inside an instruction rounds (or truncates) once to
    fp32 or better; the instruction's internal order is not assumed.
  * slices: the k-slices are combined by `slices` further additions (atomics in any order; the deterministic form in ascending order).
  * products of 16-bit operands are exact in fp32 (8 + 8 or 11 + 11 significand bits); FT_F32 adds one rounding per product (+1).
  * c = epilogue operations that round: alpha * acc, beta * C0 and its addition, + bias, the rank-1 fma; each is bounded by u times
    the sum of the magnitudes.  On the split paths C0 (beta = 1) and the bias take part in the slice additions: c grows by `slices`.
  * activations: relu adds nothing (Lipschitz 1).  tanhf_(x) = 1 - 2 / (__expf(2x) + 1) and sigmoidf_(x) = 1 / (1 + __expf(-x)) are
    attn_ref64's r = 1 / (X + 1) with X = e^y: relative error of X (C_EXP + C_ARG |y|) U24 (attn_ref64._r_and_err; U24 = 2^-24), then
    r (s eps_X + C_RD U24) + P_FLOOR; tanh = 1 - 2r adds its subtraction.  The pre-activation error is propagated with the Lipschitz
    constant (1 for tanh, 1/4 for sigmoid).
  * C16: half an ulp of the operand format at the result (taken at |ref| + bound), plus the fp32 bound.

Sharpness: the single-element mutations are claimed against the ROUNDED class only at K <= 2048 (SHARP_MAX_K); beyond, the bound is
as large as one product and the exact class carries that duty."""
import math

import torch

from attn_ref64 import C_ARG, C_EXP, C_RD, P_FLOOR
from attn_ref64 import U as U24

U = 2.0 ** -23
SHARP = 10.0
SHARP_MAX_K = 2048
ACT_NONE, ACT_TANH, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3
F32, BF16, F16 = 0, 1, 2
F64 = torch.float64

MUTATIONS = ("drop_k", "drop_last_step", "swap_groups", "pad_in", "no_beta", "bias_shift", "r1_compact_row", "rowmap_shift",
             "a_rows_shift", "k_shift_off", "rows_beyond")


def op_dtype(fmt):
    return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[fmt]


def round_op(x, fmt):
    """x (fp32) as the kernels of operand format `fmt` read it, in fp32"""
    x = x.float()
    return x if fmt == F32 else x.to(op_dtype(fmt)).float()


def ulp16(x, fmt):
    """spacing of the 16-bit format `fmt` at |x| (float64 tensor): bf16 8 significand bits, normal everywhere fp32 is; fp16 11 bits,
    subnormal spacing 2^-24 below 2^-14"""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126)))
    if fmt == BF16:
        return torch.exp2(e - 7)
    return torch.exp2(e.clamp(min=-14.0) - 10)


# ------------------------------------------------------------------------------------------------------------ index restatements
def row_map_ref(lens, T, B):
    """ft_rowmap_build, from the header: compact rows batch-major -- utterance b = rows (t, b), t < lens[b], then ONE separator: row
    (lens[b], b) when lens[b] < T, else -1; time-major row index t * B + b.  Returns (list, rows)."""
    m = []
    for b in range(B):
        n = max(0, min(int(lens[b]), T))
        m += [t * B + b for t in range(n)]
        m.append(n * B + b if n < T else -1)
    return m, len(m)


def chunk_gather_rows_ref(lens, T, B, t0, t1):
    """ft_chunk_gather_rows, from the header: the chunk's compact rows are row_map_ref's over clamp(lens[b] - t0, 0, t1 - t0); compact row
    i = (t, b): a_rows[i] = off_b + t0 + t, off_b = sum_{b' < b} (lens[b'] + 1), rowmap[i] = t * B + b; the chunk's separator rows are
    dropped (-1) and read a valid row of the chunk (WHICH is the kernel's choice: callers compare a_rows only where rowmap >= 0).
    Returns (a_rows, rowmap, rows), a_rows None at the separators."""
    a_rows, rmap = [], []
    off = 0
    for b in range(B):
        n = max(0, min(int(lens[b]) - t0, t1 - t0))
        for t in range(n):
            a_rows.append(off + t0 + t)
            rmap.append(t * B + b)
        a_rows.append(None)
        rmap.append(-1)
        off += int(lens[b]) + 1
    return a_rows, rmap, len(rmap)


def operands(a_src, b_src, *, M, N, K, a_km=False, b_km=False, a_off=(0, 0), b_off=(0, 0), a_rows=None, rows=None, compact=0,
             k_shift=0, mut=None, mut_arg=0):
    """The dense a [M, K] and b [N, K] a call multiplies, by plain indexing on the ROUNDED fp32 sources of its images.
    a_src / b_src: the image's source matrix ([rows][cols] as ft_bf16_image saw it; anything outside is the image's zero padding).
    k-major operand: image rows are k.  a_off / b_off = (row, col) offset of the pointer inside the image (for a k-major A with compact
    = 2 the row offset IS the k_shift the caller applied).  a_rows (+ rows): compact row m < rows reads image row a_rows[m]; rows at or
    beyond `rows` are dropped by the epilogue (zeros here).  compact = 2: k runs over compact rows, k < rows - k_shift.
    Mutations (wrong references): a_rows_shift -- a_rows entry m + 1; k_shift_off -- the reduction limit taken with k_shift + 1;
    rows_beyond -- compact = 2 without the limit; swap_groups -- rows 0..15 and 16..31 of a swapped; drop_k -- k = mut_arg missing;
    drop_last_step -- the last 32 k missing.  (pad_in is `pad_in_term`, the epilogue mutations are `reference`'s.)"""
    def window(src, km, off, R):
        # [R rows][K] with k innermost, zero where the image holds padding
        s = src.to(F64)
        if km:
            s = s.t()                                    # now [image col = row index][image row = k]
            off = (off[1], off[0])
        out = torch.zeros(R, K, dtype=F64, device=src.device)
        r1, k1 = min(R, s.shape[0] - off[0]), min(K, s.shape[1] - off[1])
        if r1 > 0 and k1 > 0:
            out[:r1, :k1] = s[off[0]:off[0] + r1, off[1]:off[1] + k1]
        return out

    if a_rows is not None:
        lst = list(a_rows[:rows])
        if mut == "a_rows_shift":
            lst = [a_rows[min(m + 1, rows - 1)] for m in range(rows)]
        s = a_src.to(F64)
        a = torch.zeros(M, K, dtype=F64, device=a_src.device)
        idx = torch.tensor([r if r is not None else 0 for r in lst], device=a_src.device, dtype=torch.long)
        a[:rows, :min(K, s.shape[1])] = s[idx][:, :K]
    else:
        a = window(a_src, a_km, a_off, M)
    b = window(b_src, b_km, b_off, N)
    if compact == 2:
        ks = k_shift + (1 if mut == "k_shift_off" else 0)
        if mut != "rows_beyond":
            lim = max(0, rows - ks)
            a[:, lim:] = 0
    if mut == "swap_groups":
        a = torch.cat([a[16:32], a[:16], a[32:]])
    elif mut == "drop_k":
        a[:, mut_arg] = 0
    elif mut == "drop_last_step":
        a[:, max(0, K - 32):] = 0
    return a, b


def pad_in_term(a_wide, a_off, M, K, b):
    """mutation pad_in: the element of a's NEIGHBOUR region at k = K (the column of the wider source just beyond the view) enters the
    product as if the partner held b[:, K - 1] there instead of zero padding.  [M, N] float64, to be added to the dot."""
    col = a_wide.to(F64)[a_off[0]:a_off[0] + M, a_off[1] + K]
    return col[:, None] * b[:, K - 1][None, :]


# ------------------------------------------------------------------------------------------------------------ reference and bound
def _act(x, act):
    if act == ACT_TANH:
        return torch.tanh(x)
    if act == ACT_RELU:
        return x.clamp(min=0)
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    return x


def _act_err(pre, dpre, act):
    if act in (ACT_NONE, ACT_RELU):
        return dpre
    y = 2.0 * pre if act == ACT_TANH else -pre               # X = e^y, r = 1 / (X + 1)
    r, s = torch.sigmoid(-y), torch.sigmoid(y)
    dr = r * (s * (C_EXP + C_ARG * y.abs()) * U24 + C_RD * U24) + P_FLOOR
    if act == ACT_TANH:
        return 2.0 * dr + U24 + dpre                          # 1 - 2 r: the subtraction; Lipschitz 1
    return dr + 0.25 * dpre


def reference(a, b, *, alpha=1.0, beta=0.0, C0=None, bias=None, r1_row=None, r1_col=None, act=ACT_NONE, rowmap=None, rows=None,
              c16=None, fmt=BF16, slices=1, split=False, pad_term=None, mut=None, k_len=None):
    """a [M, K], b [N, K] float64 (from `operands`).  C0 [Rows, N] = the output matrix before the call (its untouched rows come back
    as they are); rowmap (list) + rows: compact row m < rows goes to output row rowmap[m] (negative: dropped); None: row m.
    slices / split: the k-slices of the plan and whether they are combined by additions (atomics or the deterministic reduction).
    k_len: the reduction length the kernel really walks when that is not K (compact = 2: *rows_dev - k_shift of the capacity K).
    c16: the 16-bit format the result is rounded to, or None.  pad_term: float64 [M, N] added to the dot (mutation pad_in).
    Returns (ref, bound) float64 of C0's shape; bound is +inf nowhere and 0 on untouched elements (they must come back EQUAL)."""
    M, K = a.shape
    N = b.shape[0]
    dev = a.device
    dot = a @ b.t()
    absdot = a.abs() @ b.abs().t()
    if pad_term is not None:
        dot = dot + pad_term
    if C0 is None:
        C0 = torch.zeros(M, N, dtype=F64, device=dev)
    C0 = C0.to(F64)
    if rowmap is None:
        src = torch.arange(M, device=dev)
        dst = src
    else:
        rm = list(rowmap)
        if mut == "rowmap_shift":
            rm = [rm[min(m + 1, rows - 1)] for m in range(rows)]
        pairs = [(m, rm[m]) for m in range(rows) if rm[m] >= 0]
        src = torch.tensor([p[0] for p in pairs], device=dev, dtype=torch.long)
        dst = torch.tensor([p[1] for p in pairs], device=dev, dtype=torch.long)
    ref = C0.clone()
    bound = torch.zeros_like(C0)
    if src.numel() == 0:
        return ref, bound
    d, ad, c0 = dot[src], absdot[src], C0[dst]
    t_dot = alpha * d
    t_c = (beta * c0) if (beta != 0.0 and mut != "no_beta") else torch.zeros_like(c0)
    bv = torch.zeros(N, dtype=F64, device=dev)
    if bias is not None:
        bv = bias.to(F64)
        if mut == "bias_shift":
            bv = torch.roll(bv, -1)
    t_r1 = torch.zeros_like(c0)
    if r1_row is not None:
        rr = r1_row.to(F64)[src if mut == "r1_compact_row" else dst]
        t_r1 = rr[:, None] * r1_col.to(F64)[None, :]
    pre = t_dot + t_c + bv[None, :] + t_r1
    P = 4 if fmt == F32 else 32
    n_instr = -(-(-(-(K if k_len is None else k_len) // slices)) // P)
    n_sum = n_instr + P + (slices if split else 0) + (1 if fmt == F32 else 0)
    c = 1 + (2 if beta != 0.0 else 0) + (1 if bias is not None else 0) + (1 if r1_row is not None else 0) + (slices if split else 0)
    mag = t_dot.abs() + ((beta * c0).abs() if beta != 0.0 else 0.0) + bv.abs()[None, :] + t_r1.abs()
    dpre = U * (n_sum * abs(alpha) * ad + c * mag)
    out = _act(pre, act)
    err = _act_err(pre, dpre, act)
    if c16 is not None:
        err = err + 0.5 * ulp16(out.abs() + err, c16)
    ref[dst] = out
    bound[dst] = err
    return ref, bound


def ratio(got, ref, bound):
    """largest |got - ref| / bound; elements with bound 0 must be equal (ratio inf otherwise); NaN counts as inf"""
    d = (got.to(F64) - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    r = torch.where(bound > 0, d / bound.clamp(min=1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(r.max()) if r.numel() else 0.0


def exact_round(ref, c16):
    """the exact-class reference as the kernel must return it: fp32 (the value is representable), or its one RNE rounding to the 16-bit
    format.  float64 -> 16 bits directly: one rounding."""
    return ref.to(torch.float32) if c16 is None else ref.to(op_dtype(c16))


# ------------------------------------------------------------------------------------------------------------ input classes
SPECIALS = (1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3e-6, -3e-6, 6.0e-8, 65504.0, 65519.0, -65519.0)


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def exact_matrix(rows, cols, seed):
    """integers in [-8, 8] as fp32 (CPU)"""
    return torch.randint(-8, 9, (rows, cols), generator=_gen(seed)).float()


def exact_vector(n, seed, lim=5):
    return torch.randint(-lim, lim + 1, (n,), generator=_gen(seed)).float()


def assert_exact_case(a, b, alpha, beta=0.0, C0=None, bias=None, r1_row=None, r1_col=None):
    """the condition under which the exact class IS exact: every partial sum is a multiple of `unit` with fewer than 2^24 of them"""
    def pow2(v):
        return v != 0.0 and math.frexp(abs(v))[0] == 0.5
    assert pow2(alpha) and (beta == 0.0 or pow2(beta))
    unit = min([abs(alpha), 1.0] + ([abs(beta)] if beta != 0.0 else []))
    tot = abs(alpha) * float(a.abs().max()) * float(b.abs().max()) * a.shape[1]       # >= alpha sum_k |a||b| of every element (cheap at any size)
    if C0 is not None and beta != 0.0:
        tot += abs(beta) * float(C0.abs().max())
    if bias is not None:
        tot += float(bias.abs().max())
    if r1_row is not None:
        tot += float(r1_row.abs().max()) * float(r1_col.abs().max())
    assert tot / unit < 2.0 ** 24, (tot, unit)
    for t in (a, b, C0, bias, r1_row, r1_col):
        assert t is None or bool((t == t.round()).all())
    assert float(a.abs().max()) <= 8 and float(b.abs().max()) <= 8


def rounded_matrix(rows, cols, seed, zeros=False, specials=True):
    """N(0, 1) with SPECIALS planted along the first row (where they fit) and in a column; zeros=True: a sprinkle of exact zeros
    (staging path: the rounding happens in the kernel)"""
    g = _gen(seed)
    x = torch.randn(rows, cols, generator=g)
    if specials:
        n = min(len(SPECIALS), cols)
        x[0, :n] = torch.tensor(SPECIALS[:n])
        n = min(len(SPECIALS), rows - 1)
        if n > 0:
            x[1:1 + n, cols // 2] = torch.tensor(SPECIALS[:n])
    if zeros:
        x[torch.rand(rows, cols, generator=g) < 0.05] = 0.0
    return x


# ------------------------------------------------------------------------------------------------------------ emulated accumulation
def emulate(a32, b32, alpha, order="fwd", slices=1, seed=0):
    """fp32 stand-in for a kernel (CPU tests): alpha * a b^T accumulated in 32-wide k chunks in the given chunk order, the chunks dealt to
    `slices` partial sums that are added at the end.  a32 [M, K], b32 [N, K] fp32."""
    K = a32.shape[1]
    chunks = [(k, min(k + 32, K)) for k in range(0, K, 32)]
    if order == "rev":
        chunks = chunks[::-1]
    elif order == "shuffle":
        perm = torch.randperm(len(chunks), generator=_gen(seed)).tolist()
        chunks = [chunks[i] for i in perm]
    per = -(-len(chunks) // slices)
    total = None
    for s in range(0, len(chunks), per):
        acc = torch.zeros(a32.shape[0], b32.shape[0], dtype=torch.float32)
        for k0, k1 in chunks[s:s + per]:
            acc = acc + a32[:, k0:k1] @ b32[:, k0:k1].t()
        part = torch.tensor(alpha, dtype=torch.float32) * acc
        total = part if total is None else total + part
    return total


# ------------------------------------------------------------------------------------------------------------ gemv over compact rows
def gemv_rows_ref(x, w, bias, rowmap, rows, lens, T, B, y0, fmt):
    """ft_img_gemv_rows: y[rowmap[c]] = sum_k x[c][k] op16(w[k]) + bias for c < rows (negative: skipped); the separator row of utterance b
    (t == lens[b]) also gives its value to every later frame of b.  x [rows.., K] = the ROUNDED image rows (float64-able), y0 [T*B] the
    output before the call.  Bound: the 64-lane strided fma chain (ceil(K / 512) * 8 fmas per lane) + the 6-level butterfly + the bias."""
    xd, wd = x.to(F64), round_op(w, fmt).to(F64)
    K = wd.numel()
    ref, bound = y0.to(F64).clone(), torch.zeros(y0.numel(), dtype=F64, device=y0.device)
    depth = -(-K // 512) * 8 + 6 + 1
    bv = float(bias) if bias is not None else 0.0
    for c in range(rows):
        d = rowmap[c]
        if d < 0:
            continue
        v = float((xd[c, :K] * wd).sum()) + bv
        e = U * depth * (float((xd[c, :K] * wd).abs().sum()) + abs(bv))
        t, b = divmod(d, B)
        ref[d], bound[d] = v, e
        if t == max(0, int(lens[b])):
            for tt in range(t + 1, T):
                ref[tt * B + b], bound[tt * B + b] = v, e
    return ref, bound


def gemv_rows_bwd_ref(x, dy, rowmap, rows, dw0, db0, rpb=256):
    """ft_img_gemv_rows_bwd: dw[k] = dw0[k] + sum_c dy[rowmap[c]] x[c][k], db = db0 + sum_c dy[rowmap[c]] (c < rows, rowmap >= 0).
    Bound: a block's rpb-row fma chain, then one atomic per block onto dw (db: a 64-lane strided sum + butterfly per block)."""
    xd = x.to(F64)[:rows]
    d = torch.tensor([float(dy[rowmap[c]]) if rowmap[c] >= 0 else 0.0 for c in range(rows)], dtype=F64, device=x.device)
    blocks = -(-max(rows, 1) // rpb)
    dw = dw0.to(F64) + d @ xd
    adw = dw0.to(F64).abs() + d.abs() @ xd.abs()
    db = float(db0) + float(d.sum())
    adb = abs(float(db0)) + float(d.abs().sum())
    return dw, U * (min(rows, rpb) + blocks) * adw, db, U * (-(-min(rows, rpb) // 64) + 6 + blocks) * adb


def emulate_call(a64, b64, *, alpha, beta=0.0, C0=None, bias=None, r1_row=None, r1_col=None, rowmap=None, rows=None, order="fwd", slices=1,
                 seed=0, relu=False):
    """fp32 stand-in for a whole call (CPU tests): `emulate`'s accumulation, then the kernels' epilogue in fp32 (alpha acc + beta C0 + bias
    + r1, optional relu) scattered through the row map.  a64 / b64 hold values the operand format represents (from `operands`)."""
    f32 = torch.float32
    v = emulate(a64.to(f32), b64.to(f32), alpha, order, slices, seed)
    M, N = v.shape
    out = (C0 if C0 is not None else torch.zeros(M, N)).to(f32).clone()
    pairs = [(m, m) for m in range(M)] if rowmap is None else [(m, rowmap[m]) for m in range(rows) if rowmap[m] >= 0]
    for m, d in pairs:
        x = v[m]
        if beta != 0.0:
            x = x + torch.tensor(beta, dtype=f32) * out[d]
        if bias is not None:
            x = x + bias.to(f32)
        if r1_row is not None:
            x = x + r1_row.to(f32)[d] * r1_col.to(f32)
        out[d] = x.clamp(min=0) if relu else x
    return out
