"""Float64 restatement of the encoder convolution in its split-image mode -- ops.conv_norm_relu and ops.LinearFn with
mode = ("split3", fmt, fmt) -- with input classes, per-element bounds, the derived GRADE of the split product and the wrong references
of the sensitivity checks (imported by tests/test_conv_ref64_cpu.py and tests/test_gpu_encoder_conv_f64.py, not collected).  Composed
from elementwise_ref64 (im2col, col2im, instnorm_fwd, instnorm_bwd, colsum) and gemm_ref64 (round_op, reference, emulate_call); plain
torch on whatever device the inputs live on; nothing here calls the project's kernels.

The split (comments of csrc/gemm_bf16.hip):  hi = op16(x),  lo = op16(fp32(x - hi)).  An ACTIVATION image is [hi | lo | hi], a WEIGHT
image [hi | hi | lo], three column blocks of K; the image is [Rp][Cp] with Rp = ceil256(R + 32), Cp = ceil256(3 K), rows [R, Rp) and
columns [3 K, Cp) zero.  ONE 16-bit GEMM over the 3 K columns then gives

    y[r][n] = sum_k ( x_hi w_hi + x_lo w_hi + x_hi w_lo ) + bias[n]                                   ("the three-term formula")

FORWARD WITH THE KERNEL'S OWN ROUNDING (`forward`): that formula on the split of the float64 im2col matrix, under gemm_ref64's bound at
reduction length 3 K with the slices of the call's plan.  In fp16 the magnitudes of the bound's sum are taken through
cumm_ref64.lifted: ASSUMPTION ABOUT THE MATRIX INSTRUCTION, from that module's measurement -- a SUBNORMAL fp16 operand is aligned as
if it carried the exponent of the smallest normal 2^-14, so the additions inside an instruction round relative to the lifted
magnitude.  (A weight of size 0.03 has lo ~ 1.5e-5 < 2^-14: EVERY weight lo operand of the encoder is an fp16 subnormal.)

BACKWARD (`linear_bwd`, then elementwise_ref64.col2im / instnorm_bwd from the device's own intermediate gradients, each stage under the
bound its module already has):  dcol = op16(dpre) . op16(W);  dW = op16(dpre)^T . op16(col), the [hi] blocks viewed in place, atomic
split-K into a zeroed output (beta = 1);  db = the fp32 column sums of dpre.  The fallbacks LinearFn takes by shape -- K % 32 != 0, or
rows N K < 2^20 -- run the forward as the fp32 staging GEMM on the WRITTEN column matrix (`forward_f32`) and the backward on 16-bit
operands all the same (plain images, or the staging kernel that rounds as it loads): same formulas, gemm_ref64's bound of that path.

THE GRADE (`grade_bound`): how far the three-term formula itself is from the true x . w.  With u = the format's unit roundoff (bf16
2^-8, fp16 2^-11) and f = half its subnormal spacing (fp16 2^-25; bf16: none above fp32's own), write x = x_hi + x_lo + r_x:
    |x_lo| <= l(x) = max(u |x|, f)      (x - hi is at most half a spacing of x, and exact in fp32)
    |r_x|  <= r(x) = u l(x) + f         (the rounding of x - hi: relative where lo is normal, f where it is subnormal)
    x w - (x_hi w_hi + x_lo w_hi + x_hi w_lo) = x_lo w_lo + r_x w + (x_hi + x_lo) r_w
    |...| <= l(x) l(w) + r(x) |w| + (|x| + r(x)) r(w)
-- three terms of order u^2 |x w| plus the absolute floor f (|x| + |w|) per product; summed over k.  Derived, not fitted.  Precondition
|x| < 65520 in fp16 (beyond, hi is infinite).  At |w| ~ 1e-4 in fp16 the floor IS the bound: 2^-25 / 1e-4 = 3e-4 of each product,
the size of the plain 16-bit rounding -- the split gains nothing there, and this bound says so.

INPUT CLASSES
  split-exact  x = a + b 2^-13 and w alike, a, b in {-1, 0, 1}, b = 0 where a = 0.  Then hi = a and lo = b 2^-13 EXACTLY in both formats
               (2^-13 is below half a spacing on either side of +-1 in fp16 -- 2^-12 below 1 -- and a normal fp16 number; 2^-10 would NOT
               do: fp16 represents 1 + 2^-10, so hi would not be a), every product of the three-term formula is a multiple of 2^-13 and
               the sum of ALL magnitudes is below 2^24 of them (`assert_split_exact`, from the data itself): every partial sum in any
               order or split is exact in fp32 and a correct kernel equals the reference BIT FOR BIT.  Carries 3 K = 7680 with split-K.
  rounded      N(0, 1) data; gemm_ref64.SPECIALS (ties of both formats, fp16 subnormals, the overflow edge 65504 / 65519) planted in
               one frame of the LAST utterance and in weight row 0 (weights scaled by the power of two 2^-4: ties stay ties); utterance 0
               and weight row 1 positive with every residue x - hi = +0.45 of a spacing, so that a dropped correction term adds up
               coherently in output column 1 of utterance 0's rows.
  Both: rows behind an utterance's length hold +-3e4 (finite, inside the tensor), which nothing may read.

MUTATIONS (wrong references; each must lie >= SHARP bounds away at the shapes that claim it, tests/test_conv_ref64_cpu.py):
  drop_xlo_whi / drop_xhi_wlo  a correction term missing;   act_layout_hhl  the activation laid out [hi | hi | lo];   drop_k  one k of
  K missing (all three blocks);   tap_shift  the taps one frame off (elementwise_ref64's im2col_shift);   len_plus_one  a tap read one
  frame behind lens[b];   no_bias;   dw_hi_plus_lo  a dW that reads hi + lo (the unrounded column matrix) instead of hi."""
import torch

import elementwise_ref64 as E
import gemm_ref64 as R
from cumm_ref64 import lifted

U = R.U
SHARP = R.SHARP
F64 = torch.float64
BF16, F16, F32 = R.BF16, R.F16, R.F32
U16 = {BF16: 2.0 ** -8, F16: 2.0 ** -11}                 # unit roundoff: half a spacing relative to the binade's lower end
HALF_SUB = {BF16: 0.0, F16: 2.0 ** -25}                  # half the subnormal spacing (bf16's lies at fp32's own underflow: not reached)
Q_EXACT = 13                                             # the split-exact class's lo unit is 2^-13
GARBAGE = 3.0e4
W_SCALE = 2.0 ** -4
COHERENT = 0.45                                          # residue of the coherent rows, in spacings of the 16-bit format

MUT_FWD = ("drop_xlo_whi", "drop_xhi_wlo", "act_layout_hhl", "drop_k", "tap_shift", "len_plus_one", "no_bias")
MUT_BWD = ("dw_hi_plus_lo",)
MUTATIONS = MUT_FWD + MUT_BWD


def up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------------ split and layout
def split(x, fmt):
    """(hi, lo) fp32 of the fp32 tensor x: hi = op16(x), lo = op16(fp32(x - hi))"""
    x = x.float()
    hi = R.round_op(x, fmt)
    return hi, R.round_op((x - hi).float(), fmt)


def split_blocks(src, fmt, weight, layout=None):
    """the three column blocks [R, 3 K] float64 of the split image of src [R, K]; layout: "hlh" / "hhl" (default: by `weight`)"""
    hi, lo = split(src, fmt)
    layout = layout or ("hhl" if weight else "hlh")
    return torch.cat([{"h": hi, "l": lo}[c] for c in layout], 1).to(F64)


def image_dims(R_, K3):
    """(Rp, Cp) of an operand image of R_ rows and K3 columns"""
    return up(R_ + 32, 256), up(K3, 256)


def split_image(src, fmt, weight):
    """the whole [Rp][Cp] split image of src [R, K], float64, padding included"""
    R_, K = src.shape
    Rp, Cp = image_dims(R_, 3 * K)
    out = torch.zeros(Rp, Cp, dtype=F64, device=src.device)
    out[:R_, :3 * K] = split_blocks(src, fmt, weight)
    return out


def plain_image(src, fmt):
    """the [Rp][Cp] plain image of src [R, K] (ft_bf16_image), float64"""
    R_, K = src.shape
    Rp, Cp = image_dims(R_, K)
    out = torch.zeros(Rp, Cp, dtype=F64, device=src.device)
    out[:R_, :K] = R.round_op(src, fmt).to(F64)
    return out


# ------------------------------------------------------------------------------------------------------------ forward
def column_matrix(x, lens, KW, mut=None):
    """the im2col matrix [L B, C KW] float64 of x [L, B, C] (fp32 values, copied exactly)"""
    Lx = x.shape[0]
    ln = lens.long()
    if mut == "len_plus_one":
        ln = (ln + 1).clamp(max=Lx)
    col, _ = E.im2col(x, ln, KW, mut="im2col_shift" if mut == "tap_shift" else None)
    return col.reshape(Lx * x.shape[1], -1)


def assert_nothing_read_behind(x, lens, KW, col):
    """the reference itself must not depend on what lies behind a length: the same matrix from x with those rows zeroed"""
    m = E.frame_mask(lens.to(x.device), x.shape[0])[:, :, None]
    assert torch.equal(column_matrix(x * m, lens, KW), col)
    assert bool((x * ~m).abs().sum() > 0) or bool(m.all())


def _lift_extra(a, b, fmt, K, slices, split_sum):
    """what `lifted` adds to gemm_ref64's bound: the additions of the chain round relative to the lifted magnitudes (fp16 only)"""
    if fmt != F16:
        return 0.0
    n_instr = -(-(-(-K // slices)) // 32)
    n_sum = n_instr + 32 + (slices if split_sum else 0)
    return U * n_sum * (lifted(a, fmt) @ lifted(b, fmt).t() - a.abs() @ b.abs().t()).clamp(min=0.0)


def gemm16(a, b, fmt, *, bias=None, beta=0.0, C0=None, slices=1, split_sum=False):
    """gemm_ref64.reference (alpha = 1) on operands that hold 16-bit values, with the fp16 subnormal weighing added to its bound"""
    ref, bound = R.reference(a, b, alpha=1.0, beta=beta, C0=C0, bias=bias, fmt=fmt, slices=slices, split=split_sum)
    return ref, bound + _lift_extra(a, b, fmt, a.shape[1], slices, split_sum)


def forward_operands(col, W, fmt, mut=None, k_drop=0):
    """the dense [rows, 3 K] and [N, 3 K] float64 operands of the split forward GEMM; col [rows, K] float64 of fp32 values, W [N, K] fp32"""
    a = split_blocks(col.float(), fmt, False, layout="hhl" if mut == "act_layout_hhl" else None)
    b = split_blocks(W, fmt, True)
    K = W.shape[1]
    if mut == "drop_xlo_whi":
        a[:, K:2 * K] = 0
    elif mut == "drop_xhi_wlo":
        b[:, 2 * K:] = 0
    elif mut == "drop_k":
        a[:, k_drop::K] = 0
    return a, b


def forward(col, W, bias, fmt, *, slices=1, split_sum=False, mut=None, k_drop=0):
    """the split forward with the kernel's own rounding: (ref, bound) [rows, N] float64"""
    a, b = forward_operands(col, W, fmt, mut, k_drop)
    return gemm16(a, b, fmt, bias=None if mut == "no_bias" else bias, slices=slices, split_sum=split_sum)


def forward_f32(col, W, bias, mut=None, k_drop=0):
    """the fallback forward: the fp32 staging GEMM (FT_F32) on the written column matrix"""
    a, b = col.clone(), W.to(F64)
    if mut == "drop_k":
        a[:, k_drop] = 0
    return R.reference(a, b, alpha=1.0, bias=None if mut == "no_bias" else bias, fmt=F32)


def true_product(col, W, bias):
    y = col @ W.to(F64).t()
    return y if bias is None else y + bias.to(F64)[None, :]


def plain16(col, W, bias, fmt):
    """the plain 16-bit forward's value (mode = fmt): op16(col) . op16(W) + bias, float64"""
    return true_product(R.round_op(col.float(), fmt).to(F64), R.round_op(W, fmt), bias)


# ------------------------------------------------------------------------------------------------------------ the grade
def _lo_bound(v, fmt):
    z = torch.zeros_like(v)
    return torch.where(v > 0, (U16[fmt] * v).clamp(min=HALF_SUB[fmt]), z)


def _res_bound(v, fmt):
    z = torch.zeros_like(v)
    return torch.where(v > 0, U16[fmt] * _lo_bound(v, fmt) + HALF_SUB[fmt], z)


def grade_bound(col, W, fmt):
    """per output element, a bound on |three-term formula - true product| (docstring): [rows, N] float64"""
    x, w = col.to(F64).abs(), W.to(F64).abs()
    if fmt == F16:
        assert float(x.max()) < 65520.0 and float(w.max()) < 65520.0
    lx, lw, rx, rw = _lo_bound(x, fmt), _lo_bound(w, fmt), _res_bound(x, fmt), _res_bound(w, fmt)
    return lx @ lw.t() + rx @ w.t() + (x + rx) @ rw.t()


def share(dev, col, W):
    """largest |dev| as a share of sum_k |x w| of its element"""
    mag = col.to(F64).abs() @ W.to(F64).abs().t()
    return float((dev.abs() / mag.clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------------------------------------ backward
def linear_bwd(dpre, W, col, fmt, *, dx_slices=1, dx_split=False, dw_slices=1, dw_split=False, dw_beta=1.0, mut=None):
    """dpre [rows, N] fp32 (the device's own), W [N, K] fp32, col [rows, K] float64 of fp32 values.
    Returns {"dcol", "dW", "db"} -> (ref, bound)"""
    d16 = R.round_op(dpre, fmt).to(F64)
    w16 = R.round_op(W, fmt).to(F64)
    c16 = col if mut == "dw_hi_plus_lo" else R.round_op(col.float(), fmt).to(F64)
    out = {"dcol": gemm16(d16, w16.t().contiguous(), fmt, slices=dx_slices, split_sum=dx_split)}
    zero = torch.zeros(W.shape, dtype=F64, device=W.device)
    out["dW"] = gemm16(d16.t().contiguous(), c16.t().contiguous(), fmt, beta=dw_beta, C0=zero, slices=dw_slices, split_sum=dw_split)
    out["db"] = E.colsum(dpre)
    return out


# ------------------------------------------------------------------------------------------------------------ input classes
def lengths(Lx, B, seed):
    """ragged, always with Lx (utterance 0) and 1 (utterance 1); B = 1: [Lx]"""
    if B == 1:
        return [Lx]
    g = R._gen(seed)
    return [Lx, 1] + [int(v) for v in torch.randint(1, Lx + 1, (B - 2,), generator=g)]


def _garbage(x, lens):
    Lx, B, _ = x.shape
    behind = torch.arange(Lx)[:, None] >= torch.tensor(lens)[None, :]
    g = torch.full_like(x, GARBAGE)
    g[:, :, ::2] = -GARBAGE
    return torch.where(behind[:, :, None], g, x)


def _exact_values(shape, seed):
    g = R._gen(seed)
    a = torch.randint(-1, 2, shape, generator=g).float()
    b = torch.randint(-1, 2, shape, generator=g).float() * (a != 0)
    return a + b * 2.0 ** -Q_EXACT


def exact_inputs(Lx, B, Cin, Cout, KW, lens, seed):
    """(x [L, B, Cin], W [Cout, Cin KW], bias [Cout]) fp32, CPU, of the split-exact class"""
    x = _garbage(_exact_values((Lx, B, Cin), seed), lens)
    return x, _exact_values((Cout, Cin * KW), seed + 1), R.exact_vector(Cout, seed + 2)


def assert_split_exact(col, W, bias):
    """the condition under which the split-exact class IS exact, from the data: in BOTH formats hi is the integer part and lo the
    multiple of 2^-13, and the sum of the magnitudes of all products and the bias is below 2^24 units of 2^-13"""
    unit = 2.0 ** -Q_EXACT
    worst = 0.0
    for fmt in (BF16, F16):
        for t in (col.float(), W.float()):
            hi, lo = split(t, fmt)
            a = t.round()
            assert torch.equal(hi, a) and torch.equal(lo, t - a) and bool(((lo / unit) == (lo / unit).round()).all())
            assert float(a.abs().max()) <= 1 and float(lo.abs().max()) <= unit
        a, b = forward_operands(col.to(F64), W, fmt)
        tot = a.abs() @ b.abs().t() + (bias.to(F64).abs()[None, :] if bias is not None else 0.0)
        worst = max(worst, float(tot.max()))
    assert worst / unit < 2.0 ** 24, (worst, unit)
    assert bias is None or bool((bias == bias.round()).all())


def _coherent(shape, fmt, seed):
    """positive values whose residue x - op16(x) is +COHERENT spacings of the format"""
    v = torch.randn(shape, generator=R._gen(seed)).abs() + 0.5
    hi = R.round_op(v, fmt)
    x = hi + (COHERENT * R.ulp16(hi.to(F64), fmt)).float()
    assert torch.equal(R.round_op(x, fmt), hi)
    return x


def rounded_inputs(Lx, B, Cin, Cout, KW, lens, fmt, seed, w_scale=W_SCALE):
    """(x, W, bias) fp32, CPU, of the rounded class for operand format `fmt` (docstring)"""
    K = Cin * KW
    x = torch.randn(Lx, B, Cin, generator=R._gen(seed))
    x[:, 0] = _coherent((Lx, Cin), fmt, seed + 3)
    if B > 1:
        n = min(len(R.SPECIALS), Cin)
        x[0, B - 1, :n] = torch.tensor(R.SPECIALS[:n])
    W = R.rounded_matrix(Cout, K, seed + 1) * w_scale
    W[1] = _coherent((K,), fmt, seed + 4) * w_scale
    return _garbage(x, lens), W, torch.randn(Cout, generator=R._gen(seed + 2))


def grade_inputs(rows, N, K, w_scale, seed):
    """the data of the grade table: N(0, 1) e^N(0, 1) activations, N(0, 1) w_scale weights, no bias"""
    g = R._gen(seed)
    x = torch.randn(rows, K, generator=g) * torch.exp(torch.randn(rows, K, generator=g))
    return x, torch.randn(N, K, generator=g) * w_scale
