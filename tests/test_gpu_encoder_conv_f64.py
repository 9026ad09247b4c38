"""The encoder convolutions' split-image path against float64 (-m gpu): ops.conv_norm_relu and ops.LinearFn with
mode = ("split3", fmt, fmt), the [hi | hi | lo] weight images and the one-launch weight-image table, compared element by element with
tests/conv_ref64.py (its docstring derives every bound).  Both operand formats; paths are reached by SHAPE (CASES), never by
environment switches, and every image-GEMM case first ASSERTS its plan (ft_gemm_img_plan: image path, deterministic form, slices).

Per case: the convolution output BEFORE the norm (Im2colFn + ops.linear, composed as conv_norm_relu composes them) against the
own-rounding reference -- split-exact class: bit for bit; rounded class: ratio <= 1 of the bound --; conv_norm_relu itself equal, byte
for byte and twice, to the norm kernel applied to that output (the "det" claim); every gradient stage (norm backward, dcol, dW, db,
col2im) against its float64 restatement FROM THE DEVICE'S OWN INTERMEDIATE GRADIENTS; ops._LAZY_COLS empty after every call.  Rows
behind an utterance's length hold +-3e4 in x, which nothing may read.

Sensitivity: the device's result against the wrong references of conv_ref64.MUTATIONS at SHARP_CASES, each >= SHARP bounds away.

The grade: the split forward's deviation from the TRUE float64 product, asserted against conv_ref64.grade_bound plus the arithmetic
bound (fp16: weighed through cumm_ref64.lifted -- the assumption that the matrix instruction aligns a subnormal fp16 operand as the
smallest normal), and printed beside the plain 16-bit forward's and the float64 reference's figure for the same data.

MEASURED ON THE MI355X (profiles/encoder_conv_f64_pytest_gpu.log holds every figure): no kernel failed a case and no bug showed.
  * split-exact class: bit for bit in all 18 runs, the 15 deterministic slices of 3 K = 7680 included.
  * largest rounded-class error / bound, bf16 | fp16: convolution 0.11 | 0.13, norm 0.14 | 0.12, dpre 0.17 | 0.18, dcol 0.10 | 0.09,
    dW 0.13 | 0.08, db 0.01 | 0.01, dx 0.31 | 0.30, dgamma 0.02 | 0.03, dbeta 0.02 | 0.02; LinearFn on a 2-D activation 0.11 | 0.09.
  * closest wrong reference: a dW that reads hi + lo, 239 bounds (bf16, 259 rows) and 44 bounds (fp16) away; of the forward ones a
    dropped x_hi w_lo, 377 and 51 bounds.
  * the grade, largest share of sum |x w| at K = 320 (device split | device plain 16-bit | float64 three-term formula):
        bf16  scale 1: 4.2e-6 | 1.3e-3 | 4.2e-6     0.03: 2.8e-6 | 1.4e-3 | 2.8e-6     1e-4: 3.4e-6 | 1.4e-3 | 3.4e-6
        fp16  scale 1: 3.3e-7 | 2.1e-4 | 6.5e-8     0.03: 4.0e-7 | 2.0e-4 | 3.5e-7     1e-4: 1.0e-4 | 2.0e-4 | 1.0e-4
    the device at 0.04 - 0.23 of the derived bound.  fp16 at scale 1e-4 gains a factor two, no more: the floor of the subnormal lo.
  * the fp16 bound rests on cumm_ref64.lifted; the device stayed far enough inside it that these runs neither need nor test it.
NOT measured on the device: the four code mutations the wrong references stand for (a dropped `blk == 1` branch of
img_split3_im2col_k, a dropped `blk == 2` branch of img_split3_body, the two layouts swapped, `lens[b] + 1`); by reading the kernels each
moves the convolution output at least as far as the wrong reference next to it."""
from types import SimpleNamespace

import pytest
import torch

import conv_ref64 as C
import elementwise_ref64 as E
import gemm_ref64 as R

pytestmark = pytest.mark.gpu

FMTS = (R.BF16, R.F16)
EPS = 1e-5

# name -> shape and the path LinearFn must take for it.  rows = Lx B, K = Cin KW.
#   split: the [hi | lo | hi] x [hi | hi | lo] image GEMM over 3 K columns, the column matrix never written (lazy)
#   f32:   the fp32 staging GEMM on the written column matrix; `bwd`: what the 16-bit backward runs on ("images" / "staging")
CASES = {
    "lazy320":   dict(Lx=13, B=5, Cin=64, Cout=64, KW=5, path="split", fwd=dict(det=0, atomics=0, splits=1)),      # one partial row tile; 65 64 320 >= 2^20
    "lazy288":   dict(Lx=37, B=7, Cin=96, Cout=96, KW=3, path="split", fwd=dict(det=0, atomics=0, splits=1)),      # 259 rows cross a tile; N % 64 != 0
    "lazy_b1":   dict(Lx=53, B=1, Cin=64, Cout=64, KW=5, path="split", fwd=dict(det=0, atomics=0, splits=1)),      # B = 1
    "full":      dict(Lx=61, B=8, Cin=512, Cout=512, KW=5, path="split", fwd=dict(det=1, atomics=0, splits=lambda s: s > 1)),   # 3 K = 7680
    "small":     dict(Lx=10, B=5, Cin=64, Cout=64, KW=5, path="f32", bwd="staging"),                                # 50 64 320 < 2^20
    "k240":      dict(Lx=23, B=5, Cin=80, Cout=64, KW=3, path="f32", bwd="images"),                                 # K % 32 != 0; Cin != Cout
}
LINEAR2D = dict(rows=65, N=64, K=320)                                 # LinearFn on a plain 2-D activation: Bf16Image.split3(x2d, fmt, False)
SHARP_CASES = ("lazy320", "lazy288", "small", "k240")                 # 3 K <= gemm_ref64.SHARP_MAX_K; beyond, the exact class carries the duty
GRADE_SCALES = (1.0, 0.03, 1e-4)
# every reduction length of the forward GEMMs of this file (tests/test_conv_ref64_cpu.py proves the classes at each)
ALL_K = tuple(sorted({c["Cin"] * c["KW"] for c in CASES.values()} | {LINEAR2D["K"]}))


def dims(case):
    c = CASES[case]
    return c["Lx"], c["B"], c["Cin"], c["Cout"], c["KW"], c["Lx"] * c["B"], c["Cin"] * c["KW"]


def drop_k_of(K):
    return K // 2 + 1


def fwd_mutations(case):
    """the forward mutations that apply to a case (the fallback has no split to get wrong; B = 1 and full lengths have no frame behind)"""
    return C.MUT_FWD if CASES[case]["path"] == "split" else ("drop_k", "tap_shift", "len_plus_one", "no_bias")


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.lib()
    return L, ops


def check_plan(plan, expect, tag):
    got = (plan.tile_rows, plan.stage_k, plan.gather, plan.atomics, plan.det, plan.splits)
    print("%s plan: tile %d stage_k %d gather %d atomics %d det %d splits %d" % ((tag,) + got))
    for k, v in expect.items():
        g = getattr(plan, k)
        assert (v(g) if callable(v) else g == v), "%s: plan.%s = %d" % (tag, k, g)
    return SimpleNamespace(slices=plan.splits, split_sum=bool(plan.atomics or plan.det))


def judge(cls, got, ref, bound, tag, seen=None):
    if cls == "exact":
        want = ref.to(torch.float32)
        assert torch.equal(want.double(), ref), "%s: the exact value is not an fp32 number" % tag
        assert torch.equal(got, want), "%s exact: %d of %d elements differ, max |d| %g" % (
            tag, int((got != want).sum()), got.numel(), float((got.double() - ref).abs().max()))
        print("%s exact: equal bit for bit" % tag)
        return 0.0
    r = R.ratio(got, ref, bound)
    print("%s rounded: max |err| / bound = %.3f" % (tag, r))
    if seen is not None:
        seen.append((tag, r))
    assert r <= 1.0, "%s: error %.3f x the bound" % (tag, r)
    return r


def inputs(case, cls, fmt, seed):
    Lx, B, Cin, Cout, KW, rows, K = dims(case)
    lens = C.lengths(Lx, B, seed)
    if cls == "exact":
        x, W, bias = C.exact_inputs(Lx, B, Cin, Cout, KW, lens, seed)
    else:
        x, W, bias = C.rounded_inputs(Lx, B, Cin, Cout, KW, lens, fmt, seed)
    g = R._gen(seed + 9)
    gamma, beta = 1.0 + 0.1 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    keep = (torch.rand(Lx, B, Cout, generator=g) > 0.5).float() * 2
    dout = torch.randn(Lx, B, Cout, generator=g)
    cu = lambda t: t.cuda()
    return SimpleNamespace(lens_l=lens, lens=torch.tensor(lens, dtype=torch.int32, device="cuda"), x=cu(x), W=cu(W), bias=cu(bias), gamma=cu(gamma),
                           beta=cu(beta), keep=cu(keep), dout=cu(dout))


def forward_plan(env, case, fmt, d):
    """the plan of the forward GEMM exactly as LinearFn issues it (images of the case's own data); None on the fallback"""
    L, ops = env
    Lx, B, Cin, Cout, KW, rows, K = dims(case)
    took = K % 32 == 0 and ops.images_apply(fmt, rows, Cout, K)
    assert took == (CASES[case]["path"] == "split"), "%s: LinearFn takes another path than the table says" % case
    if not took:
        return None
    xi = ops.Bf16Image.split3_im2col(d.x, d.lens, KW, fmt)
    wi = ops.Bf16Image.of_weight(d.W, fmt, split=True)
    y = torch.empty(rows, Cout, device="cuda")
    plan = ops.gemm_img_plan(xi, 0, xi.ptr(), wi, 0, wi.ptr(), y, rows, Cout, 3 * K, Cout, bias=d.bias, splitk=ops._ENC_SPLITK)
    return check_plan(plan, CASES[case]["fwd"], "%s f%d forward" % (case, fmt))


def backward_plans(env, case, fmt, rows, N, K, kind):
    """(dx plan, dW plan) of the backward's image GEMMs, queried on blank images of the call's shapes; the staging kernel: one slice"""
    L, ops = env
    one = SimpleNamespace(slices=1, split_sum=False)
    if kind == "staging":
        return one, one
    d_img = ops.Bf16Image._blank(rows, N, fmt, "cuda")
    wide = 3 if kind == "split" else 1
    w_img = ops.Bf16Image._blank(N, wide * K, fmt, "cuda").view_cols(K)
    x_img = ops.Bf16Image._blank(rows, wide * K, fmt, "cuda").view_cols(K)
    dx, dW = torch.empty(rows, K, device="cuda"), torch.empty(N, K, device="cuda")
    p_dx = ops.gemm_img_plan(d_img, 0, d_img.ptr(), w_img, 1, w_img.ptr(), dx, rows, K, N, K, beta=0.0)
    p_dw = ops.gemm_img_plan(d_img, 1, d_img.ptr(), x_img, 1, x_img.ptr(), dW, N, K, rows, K, beta=1.0, splitk=True)
    return check_plan(p_dx, {}, "%s f%d dx" % (case, fmt)), check_plan(p_dw, {}, "%s f%d dW" % (case, fmt))


def conv_stages(env, case, fmt, d, keep):
    """Im2colFn + ops.linear + InstNormReluFn composed as conv_norm_relu composes them, with the intermediate tensors kept"""
    L, ops = env
    Lx, B, Cin, Cout, KW, rows, K = dims(case)
    mode = ("split3", fmt, fmt)
    lazy = K % 32 == 0 and ops.images_apply(fmt, rows, Cout, K)
    p = SimpleNamespace(x=d.x.clone().requires_grad_(True), W=d.W.reshape(Cout, Cin, KW).clone().requires_grad_(True),
                        bias=d.bias.clone().requires_grad_(True), gamma=d.gamma.clone().requires_grad_(True), beta=d.beta.clone().requires_grad_(True))
    col = ops.Im2colFn.apply(p.x, d.lens, KW, lazy)
    y = ops.linear(col, p.W.reshape(Cout, K), p.bias, mode=mode)
    if lazy:
        ops._materialize_col(col)
    assert not ops._LAZY_COLS, "a lazy column entry was left behind"
    out = ops.InstNormReluFn.apply(y, p.gamma, p.beta, keep, d.lens, EPS)
    p.col, p.y, p.out = col, y, out
    return p


def reference_forward(case, fmt, d, fp, mut=None):
    Lx, B, Cin, Cout, KW, rows, K = dims(case)
    col = C.column_matrix(d.x, d.lens, KW, mut=mut)
    if CASES[case]["path"] == "split":
        return C.forward(col, d.W, d.bias, fmt, slices=fp.slices, split_sum=fp.split_sum, mut=mut, k_drop=drop_k_of(K))
    return C.forward_f32(col, d.W, d.bias, mut=mut, k_drop=drop_k_of(K))


# ------------------------------------------------------------------------------------------------------------------ the convolution
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_convolution_against_float64(env, case, fmt):
    L, ops = env
    Lx, B, Cin, Cout, KW, rows, K = dims(case)
    assert K in ALL_K
    mode = ("split3", fmt, fmt)
    split_path = CASES[case]["path"] == "split"
    for cls in (("exact", "rounded") if split_path else ("rounded",)):
        d = inputs(case, cls, fmt, seed=7 * Lx + K + fmt)
        assert 1 in d.lens_l or B == 1
        assert Lx in d.lens_l
        fp = forward_plan(env, case, fmt, d)
        colm = C.column_matrix(d.x, d.lens, KW)
        C.assert_nothing_read_behind(d.x, d.lens, KW, colm)
        if cls == "exact":
            C.assert_split_exact(colm, d.W, d.bias)
        ref, bound = reference_forward(case, fmt, d, fp)
        for keep_name, keep in (("keep", d.keep), ("none", None)):
            tag = "%s f%d %s keep=%s" % (case, fmt, cls, keep_name)
            s = conv_stages(env, case, fmt, d, keep)
            torch.cuda.synchronize()
            y2d = s.y.detach().reshape(rows, Cout)
            judge(cls, y2d, ref, bound, tag + " conv")
            # the whole function: the norm kernel applied to that output, byte for byte, twice
            normed = ops.InstNormReluFn.apply(s.y.detach(), d.gamma, d.beta, keep, d.lens, EPS)
            for rep in range(2):
                whole = ops.conv_norm_relu(d.x, d.lens, d.W.reshape(Cout, Cin, KW), d.bias, d.gamma, d.beta, keep, EPS, mode=mode)
                assert not ops._LAZY_COLS, "a lazy column entry was left behind"
                assert torch.equal(whole, normed), "%s: conv_norm_relu differs from the norm of the convolution output (run %d)" % (tag, rep)
            nf = E.instnorm_fwd(s.y.detach(), d.gamma, d.beta, keep, d.lens, EPS)["y"]
            judge("rounded", whole, nf[0], nf[1], tag + " norm(y)")
            if cls == "exact":
                continue
            # gradients, stage by stage from the device's own intermediates
            saved = s.out.grad_fn.saved_tensors
            mean, rstd = saved[5].clone(), saved[6].clone()
            s.y.retain_grad()
            s.col.retain_grad()
            s.out.backward(d.dout)
            torch.cuda.synchronize()
            assert not ops._LAZY_COLS
            nb = E.instnorm_bwd(s.y.detach(), s.out.detach(), d.dout, d.gamma, keep, d.lens, mean, rstd)
            dpre = s.y.grad
            judge(cls, dpre, *nb["dx"], tag + " dpre")
            judge(cls, s.gamma.grad, *nb["dgamma"], tag + " dgamma")
            judge(cls, s.beta.grad, *nb["dbeta"], tag + " dbeta")
            kind = "split" if split_path else CASES[case]["bwd"]
            pdx, pdw = backward_plans(env, case, fmt, rows, Cout, K, kind)
            lb = C.linear_bwd(dpre.reshape(rows, Cout), d.W, colm, fmt, dx_slices=pdx.slices, dx_split=pdx.split_sum, dw_slices=pdw.slices,
                              dw_split=pdw.split_sum, dw_beta=0.0 if kind == "staging" else 1.0)
            judge(cls, s.col.grad.reshape(rows, K), *lb["dcol"], tag + " dcol")
            judge(cls, s.W.grad.reshape(Cout, K), *lb["dW"], tag + " dW")
            judge(cls, s.bias.grad, *lb["db"], tag + " db")
            dxr = E.col2im(s.col.grad, d.lens, Cin, KW)
            judge(cls, s.x.grad, *dxr, tag + " dx")
            behind = torch.arange(Lx, device="cuda")[:, None] >= d.lens[None, :]
            assert bool((s.x.grad[behind] == 0).all()), "a gradient behind a length"


@pytest.mark.parametrize("fmt", FMTS)
def test_linear_on_a_plain_2d_activation(env, fmt):
    """LinearFn's split mode without im2col: Bf16Image.split3(x2d, fmt, False); forward in both classes, the backward from the [hi] views"""
    L, ops = env
    rows, N, K = LINEAR2D["rows"], LINEAR2D["N"], LINEAR2D["K"]
    assert K % 32 == 0 and ops.images_apply(fmt, rows, N, K)
    mode = ("split3", fmt, fmt)
    for cls in ("exact", "rounded"):
        if cls == "exact":
            x, W, bias = C._exact_values((rows, K), 31), C._exact_values((N, K), 32), R.exact_vector(N, 33)
        else:
            x, W, bias = R.rounded_matrix(rows, K, 34), R.rounded_matrix(N, K, 35) * C.W_SCALE, torch.randn(N, generator=R._gen(36))
            x[2], W[1] = C._coherent((K,), fmt, 37), C._coherent((K,), fmt, 38) * C.W_SCALE
        x, W, bias = (t.cuda().requires_grad_(True) for t in (x, W, bias))
        xi, wi = ops.Bf16Image.split3(x.detach(), fmt, False), ops.Bf16Image.of_weight(W.detach(), fmt, split=True)
        plan = ops.gemm_img_plan(xi, 0, xi.ptr(), wi, 0, wi.ptr(), torch.empty(rows, N, device="cuda"), rows, N, 3 * K, N, bias=bias.detach(),
                                 splitk=ops._ENC_SPLITK)
        fp = check_plan(plan, dict(det=0, atomics=0, splits=1), "linear2d f%d forward" % fmt)
        colm = x.detach().double()
        if cls == "exact":
            C.assert_split_exact(colm, W.detach(), bias.detach())
        y = ops.linear(x, W, bias, mode=mode)
        torch.cuda.synchronize()
        assert not ops._LAZY_COLS
        ref, bound = C.forward(colm, W.detach(), bias.detach(), fmt, slices=fp.slices, split_sum=fp.split_sum)
        tag = "linear2d f%d %s" % (fmt, cls)
        judge(cls, y.detach(), ref, bound, tag + " y")
        if cls == "exact":
            continue
        dy = torch.randn(rows, N, generator=R._gen(39)).cuda()
        y.backward(dy)
        torch.cuda.synchronize()
        pdx, pdw = backward_plans(env, "linear2d", fmt, rows, N, K, "split")
        lb = C.linear_bwd(dy, W.detach(), colm, fmt, dx_slices=pdx.slices, dx_split=pdx.split_sum, dw_slices=pdw.slices, dw_split=pdw.split_sum)
        judge(cls, x.grad, *lb["dcol"], tag + " dx")
        judge(cls, W.grad, *lb["dW"], tag + " dW")
        judge(cls, bias.grad, *lb["db"], tag + " db")
        wrong = C.linear_bwd(dy, W.detach(), colm, fmt, mut="dw_hi_plus_lo")["dW"][0]
        must_be_sharp(W.grad, wrong, lb["dW"][1], "linear2d dw_hi_plus_lo f%d" % fmt)


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def must_be_sharp(got, wrong_ref, bound, what):
    r = R.ratio(got, wrong_ref, bound)
    print("sharp %s: %.1f x the bound" % (what, r))
    assert r >= C.SHARP, "%s is only %.2f x the bound away: the check would not see it" % (what, r)
    return r


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", SHARP_CASES)
def test_sensitivity(env, case, fmt):
    """the device's own convolution output (and dW) against every wrong reference that applies, under the bound of the right one"""
    L, ops = env
    Lx, B, Cin, Cout, KW, rows, K = dims(case)
    assert 3 * K <= R.SHARP_MAX_K
    d = inputs(case, "rounded", fmt, seed=7 * Lx + K + fmt)
    fp = forward_plan(env, case, fmt, d)
    s = conv_stages(env, case, fmt, d, d.keep)
    s.y.retain_grad()
    s.out.backward(d.dout)
    torch.cuda.synchronize()
    y2d = s.y.detach().reshape(rows, Cout)
    ref, bound = reference_forward(case, fmt, d, fp)
    assert R.ratio(y2d, ref, bound) <= 1.0
    closest = None
    for mut in fwd_mutations(case):
        r = must_be_sharp(y2d, reference_forward(case, fmt, d, fp, mut=mut)[0], bound, "%s %s f%d" % (case, mut, fmt))
        closest = min(closest or (r, mut), (r, mut))
    colm = C.column_matrix(d.x, d.lens, KW)
    kind = "split" if CASES[case]["path"] == "split" else CASES[case]["bwd"]
    pdx, pdw = backward_plans(env, case, fmt, rows, Cout, K, kind)
    kw = dict(dx_slices=pdx.slices, dx_split=pdx.split_sum, dw_slices=pdw.slices, dw_split=pdw.split_sum, dw_beta=0.0 if kind == "staging" else 1.0)
    dpre = s.y.grad.reshape(rows, Cout)
    right = C.linear_bwd(dpre, d.W, colm, fmt, **kw)["dW"]
    wrong = C.linear_bwd(dpre, d.W, colm, fmt, mut="dw_hi_plus_lo", **kw)["dW"][0]
    r = must_be_sharp(s.W.grad.reshape(Cout, K), wrong, right[1], "%s dw_hi_plus_lo f%d" % (case, fmt))
    closest = min(closest, (r, "dw_hi_plus_lo"))
    print("closest mutation %s f%d: %s at %.1f x the bound" % (case, fmt, closest[1], closest[0]))


# ------------------------------------------------------------------------------------------------------------------ the grade
@pytest.mark.parametrize("fmt", FMTS)
def test_grade_of_the_split_forward(env, fmt):
    """deviation from the TRUE product as the largest share of sum_k |x w|: the device's split forward, the device's plain 16-bit forward
    (mode = fmt), the float64 three-term reference and its [hi] blocks alone on the same data.  The device's split figure is asserted
    against the derived grade bound plus the arithmetic bound; it must beat the plain forward wherever the derived bound says it can
    (everywhere but fp16 at weight scale 1e-4, where the subnormal floor of lo IS the plain rounding's size)."""
    L, ops = env
    rows, N, K = LINEAR2D["rows"], LINEAR2D["N"], LINEAR2D["K"]
    print("grade f%d: %-8s %-12s %-12s %-12s %-12s %-12s" % (fmt, "scale", "dev split", "dev plain", "ref 3-term", "ref hi only", "bound"))
    for scale in GRADE_SCALES:
        x, W = C.grade_inputs(rows, N, K, scale, seed=77)
        x, W = x.cuda(), W.cuda()
        colm = x.double()
        true = C.true_product(colm, W, None)
        y_split = ops.linear(x, W, None, mode=("split3", fmt, fmt)).double()
        y_plain = ops.linear(x, W, None, mode=fmt).double()
        torch.cuda.synchronize()
        ref3, fb = C.forward(colm, W, None, fmt)
        allowed = C.grade_bound(colm, W, fmt) + fb
        fig = [C.share(t - true, colm, W) for t in (y_split, y_plain, ref3, C.plain16(colm, W, None, fmt))] + [C.share(allowed, colm, W)]
        print("grade f%d: %-8g %-12.3g %-12.3g %-12.3g %-12.3g %-12.3g" % ((fmt, scale) + tuple(fig)))
        r = R.ratio(y_split, true, allowed)
        print("grade f%d scale %g: device split forward at %.3f of the derived bound" % (fmt, scale, r))
        assert r <= 1.0
        if not (fmt == R.F16 and scale < 1e-3):
            assert fig[0] < 0.1 * fig[1], "the split forward is not a grade better than the plain one"


# ------------------------------------------------------------------------------------------------------------------ weight images
def image_values(img, fmt):
    """the whole [Rp][Cp] payload of an operand image, widened to float64"""
    Rp, Cp = C.image_dims(img.rows, img.cols)
    assert Cp == img.ld
    return img.buf[:Rp * Cp * 2].view(torch.float16 if fmt == R.F16 else torch.bfloat16).reshape(Rp, Cp).double()


def image_bits(img):
    Rp, Cp = C.image_dims(img.rows, img.cols)
    return img.buf[:Rp * Cp * 2].view(torch.int16).clone()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N,K", [(64, 320), (96, 288), (5, 8)])
def test_weight_image_equals_its_restatement(env, fmt, N, K):
    """[hi | hi | lo] of a weight, and [hi | lo | hi] of an activation, padding included"""
    L, ops = env
    W = (R.rounded_matrix(N, K, N + K) * C.W_SCALE).cuda()
    for weight in (True, False):
        img = ops.Bf16Image.of_weight(W, fmt, split=True) if weight else ops.Bf16Image.split3(W, fmt, False)
        torch.cuda.synchronize()
        got, want = image_values(img, fmt), C.split_image(W, fmt, weight)
        assert got.shape == want.shape and torch.equal(got, want), "split image (weight=%d) differs in %d places" % (weight, int((got != want).sum()))
        assert bool((want[:N, 2 * K:3 * K] if weight else want[:N, K:2 * K]).abs().sum() > 0)
    img = ops.Bf16Image.of_weight(W, fmt)
    torch.cuda.synchronize()
    assert torch.equal(image_values(img, fmt), C.plain_image(W, fmt))


class _StandIn(torch.nn.Module):
    """several weights of several shapes; a pass asks for plain and split images of them as a model's forward would"""
    SHAPES = ((64, 320), (96, 288), (64, 320), (40, 24), (130, 72))
    REQUESTS = ((0, True), (1, True), (2, True), (3, False), (4, False), (0, False), (4, True))      # (weight, split)

    def __init__(self):
        super().__init__()
        self.ws = torch.nn.ParameterList([torch.nn.Parameter((R.rounded_matrix(n, k, 11 * i + n) * C.W_SCALE).cuda()) for i, (n, k) in enumerate(self.SHAPES)])

    def run_pass(self, ops, fmt):
        ops.weight_images_begin(self)
        try:
            out, from_table = [], []
            for i, split in self.REQUESTS:
                W = self.ws[i]                             # the Parameter itself, as a model passes it: a p.data swap moves ITS address
                img = ops.Bf16Image.of_weight(W, fmt, split=split)
                from_table.append(ops._WIMG["cache"].get((W.data_ptr(), tuple(W.shape), fmt, bool(split))) is img)
                out.append(image_bits(img))
            cached = set(ops._WIMG["cache"])
        finally:
            ops.weight_images_end(self)
        torch.cuda.synchronize()
        return out, from_table, cached


@pytest.mark.parametrize("fmt", FMTS)
def test_one_launch_table_serves_current_values(env, fmt):
    """three passes of a stand-in module: the first plans, the later ones take every image from the one-launch table -- byte for byte the
    single-launch image of the CURRENT values, also after an in-place update; a weight whose storage moved is dropped from the plan"""
    L, ops = env
    m = _StandIn()

    def single():
        return [image_bits(ops.Bf16Image.split3(m.ws[i].detach(), fmt, True) if split else ops.Bf16Image(m.ws[i].detach(), mode=fmt)) for i, split in m.REQUESTS]

    first, t1, _ = m.run_pass(ops, fmt)
    assert not any(t1), "the first pass has no plan"
    second, t2, _ = m.run_pass(ops, fmt)
    assert all(t2), "the second pass must take every image from the table"
    want = single()
    for a, b, c in zip(first, second, want):
        assert torch.equal(a, c) and torch.equal(b, c)
    with torch.no_grad():
        for i, p in enumerate(m.ws):
            p.data.add_(0.37 * (i + 1) * C.W_SCALE)
    third, t3, _ = m.run_pass(ops, fmt)
    assert all(t3)
    now = single()
    for b, c, old in zip(third, now, want):
        assert torch.equal(b, c), "a stale weight image was served"
        assert not torch.equal(c, old)
    # storage moved: the old block stays allocated and is filled with other values; its plan entry must be dropped
    old = m.ws[0].data
    old_key = [(old.data_ptr(), tuple(old.shape), fmt, s) for s in (True, False)]
    m.ws[0].data = old.clone()
    old.fill_(123.0)
    assert m.ws[0].data.data_ptr() != old.data_ptr()
    fourth, t4, cached = m.run_pass(ops, fmt)
    assert not any(k in cached for k in old_key), "an image of a moved tensor's old storage was made"
    assert [t for (i, _), t in zip(m.REQUESTS, t4) if i == 0] == [False, False] and all(t for (i, _), t in zip(m.REQUESTS, t4) if i != 0)
    for b, c in zip(fourth, now):
        assert torch.equal(b, c), "a moved weight was served stale"
    fifth, t5, _ = m.run_pass(ops, fmt)
    assert all(t5), "the moved tensor is planned again at its new address"
    for b, c in zip(fifth, now):
        assert torch.equal(b, c)
