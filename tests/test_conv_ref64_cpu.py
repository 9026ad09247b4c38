"""tests/conv_ref64.py checked without a GPU: the split-exact class IS exact at every reduction length tests/test_gpu_encoder_conv_f64.py
uses, the bounds are sound against an fp32 emulation of the kernels in several summation orders, the derived grade bound holds for the
three-term formula in both formats, every wrong reference is sharp at the shapes that claim it (decided from the reference alone), the
float64 convolution is torch's conv1d under the mask, the layout restatement is right by hand, and the plans the GPU file expects are
what ft_gemm_img_plan answers (the query touches no device)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_ref64 as C
import elementwise_ref64 as E
import gemm_ref64 as R
import test_gpu_encoder_conv_f64 as G

ORDERS = ("fwd", "rev", "shuffle")
SLICES = (1, 3, 15)
FMTS = (R.BF16, R.F16)


def test_split_by_hand():
    x = torch.tensor([[1.0 + 2.0 ** -9 + 2.0 ** -14, -3.0, 0.0, 2.0 ** -13, 65519.0, 0.03, 1.0, 1.0]])
    for fmt, hi0, lo0 in ((R.BF16, 1.0, 2.0 ** -9 + 2.0 ** -14), (R.F16, 1.0 + 2.0 ** -9, 2.0 ** -14)):
        hi, lo = C.split(x, fmt)
        assert float(hi[0, 0]) == hi0 and float(lo[0, 0]) == lo0
        assert float(hi[0, 1]) == -3.0 and float(lo[0, 1]) == 0.0 and float(hi[0, 2]) == 0.0 and float(lo[0, 2]) == 0.0
    hi, lo = C.split(x, R.F16)
    assert float(hi[0, 4]) == 65504.0 and float(lo[0, 4]) == 15.0
    assert 0 < float(lo[0, 5].abs()) < 2.0 ** -14                       # a weight-sized value: lo is an fp16 subnormal
    img = C.split_image(x, R.F16, True)
    assert img.shape == (256, 256) and torch.equal(img[0, :8], hi[0].double()) and torch.equal(img[0, 8:16], hi[0].double())
    assert torch.equal(img[0, 16:24], lo[0].double()) and float(img[1:].abs().sum()) == 0 and float(img[:, 24:].abs().sum()) == 0
    act = C.split_image(x, R.F16, False)
    assert torch.equal(act[0, 8:16], lo[0].double()) and torch.equal(act[0, 16:24], hi[0].double())
    assert C.image_dims(225, 7680) == (512, 7680) and C.image_dims(224, 864) == (256, 1024)


@pytest.mark.parametrize("K", G.ALL_K)
def test_split_exact_class_is_exact_in_any_order_and_split(K):
    """fp32 accumulation of the 3 K columns in 32-wide chunks, forward / reverse / shuffled, in 1, 3 and 15 slices, then the fp32 bias
    addition: torch.equal with the float64 three-term reference, in both formats"""
    M, N = 9, 7
    col, W, bias = C._exact_values((M, K), K), C._exact_values((N, K), K + 1), R.exact_vector(N, K + 2)
    C.assert_split_exact(col.double(), W, bias)
    for fmt in FMTS:
        ref, _ = C.forward(col.double(), W, bias, fmt)
        assert torch.equal(ref, ref.float().double()), "the exact value is not an fp32 number"
        a, b = C.forward_operands(col.double(), W, fmt)
        for order in ORDERS:
            for sl in SLICES:
                got = R.emulate_call(a, b, alpha=1.0, bias=bias, order=order, slices=sl, seed=K)
                assert torch.equal(got, ref.float()), (K, fmt, order, sl)
        wrong, _ = C.forward(col.double(), W, bias, fmt, mut="drop_xhi_wlo")
        assert not torch.equal(wrong, ref)


def test_split_exact_class_refuses_what_is_not_exact():
    col, W = C._exact_values((4, 64), 1), C._exact_values((4, 64), 2)
    C.assert_split_exact(col.double(), W, None)
    bad = col.clone()
    bad[0, 0] = 1.0 + 2.0 ** -10                           # fp16 represents it: hi is not the integer part
    with pytest.raises(AssertionError):
        C.assert_split_exact(bad.double(), W, None)
    with pytest.raises(AssertionError):
        C.assert_split_exact(torch.ones(2, 1 << 12).double(), torch.ones(2, 1 << 12), None)      # 4096 units of 2^13: 2^25 of 2^-13


@pytest.mark.parametrize("fmt", FMTS)
def test_full_width_exact_inputs_meet_the_precondition(fmt):
    """the GPU file's largest case, from its own generator: 3 K = 7680"""
    Lx, B, Cin, Cout, KW, rows, K = G.dims("full")
    lens = C.lengths(Lx, B, 7 * Lx + K + fmt)
    x, W, bias = C.exact_inputs(Lx, B, Cin, Cout, KW, lens, 7 * Lx + K + fmt)
    col = C.column_matrix(x, torch.tensor(lens), KW)
    C.assert_nothing_read_behind(x, torch.tensor(lens), KW, col)
    C.assert_split_exact(col, W, bias)


@pytest.mark.parametrize("fmt", FMTS)
def test_bounds_are_sound_against_an_fp32_emulation(fmt):
    """forward (split, 3 K columns) and the backward's two GEMMs, emulated in fp32 in three chunk orders and several slice counts"""
    worst = 0.0
    for K in G.ALL_K:
        M, N = 12, 11
        col = R.rounded_matrix(M, K, K)
        col[2] = C._coherent((K,), fmt, K + 5)
        W, bias = R.rounded_matrix(N, K, K + 1) * C.W_SCALE, torch.randn(N, generator=R._gen(K + 2))
        a, b = C.forward_operands(col.double(), W, fmt)
        for sl in SLICES:
            ref, bound = C.forward(col.double(), W, bias, fmt, slices=sl, split_sum=sl > 1)
            for order in ORDERS:
                got = R.emulate_call(a, b, alpha=1.0, bias=bias, order=order, slices=sl, seed=K)
                worst = max(worst, R.ratio(got, ref, bound))
        ref, bound = C.forward_f32(col.double(), W, bias)
        worst = max(worst, R.ratio(R.emulate_call(col.double(), W.double(), alpha=1.0, bias=bias), ref, bound))
        dpre = torch.randn(M, N, generator=R._gen(K + 3))
        d16, w16, c16 = (R.round_op(t, fmt).double() for t in (dpre, W, col))
        for sl in (1, 3):
            lb = C.linear_bwd(dpre, W, col.double(), fmt, dx_slices=sl, dx_split=sl > 1, dw_slices=sl, dw_split=sl > 1)
            for order in ORDERS:
                worst = max(worst, R.ratio(R.emulate_call(d16, w16.t().contiguous(), alpha=1.0, order=order, slices=sl), *lb["dcol"]))
                worst = max(worst, R.ratio(R.emulate_call(d16.t().contiguous(), c16.t().contiguous(), alpha=1.0, beta=1.0, C0=torch.zeros(N, K),
                                                          order=order, slices=sl), *lb["dW"]))
            worst = max(worst, R.ratio(dpre.sum(0), *lb["db"]))
    print("fmt %d: largest emulated |err| / bound = %.3f" % (fmt, worst))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("fmt", FMTS)
def test_grade_bound_holds_for_the_three_term_formula(fmt):
    """|three-term formula - true product| <= grade_bound element by element at weight scales 1, 0.03 and 1e-4, and the bound is no
    blanket: the [hi] blocks alone miss it wherever the split gains anything"""
    rows, N, K = G.LINEAR2D["rows"], G.LINEAR2D["N"], G.LINEAR2D["K"]
    print("grade (float64 reference) f%d: %-8s %-12s %-12s %-12s" % (fmt, "scale", "3-term", "hi only", "bound"))
    for scale in G.GRADE_SCALES:
        x, W = C.grade_inputs(rows, N, K, scale, seed=77)
        col = x.double()
        true = C.true_product(col, W, None)
        a, b = C.forward_operands(col, W, fmt)
        three = a @ b.t()
        g = C.grade_bound(col, W, fmt)
        hi_only = C.plain16(col, W, None, fmt)
        fig = (C.share(three - true, col, W), C.share(hi_only - true, col, W), C.share(g, col, W))
        print("grade (float64 reference) f%d: %-8g %-12.3g %-12.3g %-12.3g" % ((fmt, scale) + fig))
        r = R.ratio(three, true, g)
        assert r <= 1.0, (scale, r)
        if fmt == R.F16 and scale < 1e-3:
            assert fig[2] > 0.1 * fig[1], "at this scale the subnormal floor is the bound: the split gains nothing and the bound says so"
        else:
            assert R.ratio(hi_only, true, g) > 1.0 and fig[2] < 0.1 * fig[1]
    # the residues at their extreme: every x and w half a spacing (minus an fp32 ulp) above a 16-bit number
    h = R.round_op(torch.rand(4, 64, generator=R._gen(9)) + 1.0, fmt)
    x = (h.double() + 0.4999 * R.ulp16(h.double(), fmt)).float()
    assert torch.equal(R.round_op(x, fmt), h)
    a, b = C.forward_operands(x.double(), x, fmt)
    assert R.ratio(a @ b.t(), C.true_product(x.double(), x, None), C.grade_bound(x.double(), x, fmt)) <= 1.0


def _case_reference(case, fmt, mut=None, data=None):
    Lx, B, Cin, Cout, KW, rows, K = G.dims(case)
    seed = 7 * Lx + K + fmt
    lens = C.lengths(Lx, B, seed)
    x, W, bias = data or C.rounded_inputs(Lx, B, Cin, Cout, KW, lens, fmt, seed)
    col = C.column_matrix(x, torch.tensor(lens), KW, mut=mut)
    if G.CASES[case]["path"] == "split":
        out = C.forward(col, W, bias, fmt, mut=mut, k_drop=G.drop_k_of(K))
    else:
        out = C.forward_f32(col, W, bias, mut=mut, k_drop=G.drop_k_of(K))
    return out, (x, W, bias), col, lens


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", G.SHARP_CASES)
def test_every_wrong_reference_is_sharp_at_the_claimed_shapes(case, fmt):
    """decided from the reference alone: each wrong reference lies >= SHARP + 1 bounds from the right one (a device result within one
    bound of the right reference is then >= SHARP bounds from the wrong one)"""
    Lx, B, Cin, Cout, KW, rows, K = G.dims(case)
    assert 3 * K <= R.SHARP_MAX_K
    (ref, bound), data, col, lens = _case_reference(case, fmt)
    C.assert_nothing_read_behind(data[0], torch.tensor(lens), KW, col)
    for mut in G.fwd_mutations(case):
        (wrong, _), _, _, _ = _case_reference(case, fmt, mut=mut, data=data)
        r = R.ratio(wrong, ref, bound)
        print("%s f%d %s: %.1f x the bound" % (case, fmt, mut, r))
        assert r >= C.SHARP + 1, (mut, r)
    # dW: a stand-in output gradient of the norm backward's scale, zero behind the lengths
    m = E.frame_mask(torch.tensor(lens), Lx)[:, :, None]
    dpre = (torch.randn(Lx, B, Cout, generator=R._gen(5)) * m).reshape(rows, Cout)
    beta = 0.0 if G.CASES[case].get("bwd") == "staging" else 1.0
    right = C.linear_bwd(dpre, data[1], col, fmt, dw_beta=beta)["dW"]
    wrong = C.linear_bwd(dpre, data[1], col, fmt, dw_beta=beta, mut="dw_hi_plus_lo")["dW"][0]
    r = R.ratio(wrong, *right)
    print("%s f%d dw_hi_plus_lo: %.1f x the bound" % (case, fmt, r))
    assert r >= C.SHARP + 1, r


def test_float64_convolution_is_conv1d_under_the_mask():
    for case in ("lazy320", "k240"):
        Lx, B, Cin, Cout, KW, rows, K = G.dims(case)
        lens = C.lengths(Lx, B, 3)
        x, W, bias = C.rounded_inputs(Lx, B, Cin, Cout, KW, lens, R.BF16, 3)
        mine = C.true_product(C.column_matrix(x, torch.tensor(lens), KW), W, bias).reshape(Lx, B, Cout)
        m = E.frame_mask(torch.tensor(lens), Lx)[:, :, None]
        xm = (x.double() * m).permute(1, 2, 0)                                  # [B, Cin, L], zero behind the lengths
        ref = F.conv1d(xm, W.double().reshape(Cout, Cin, KW), bias.double(), padding=KW // 2).permute(2, 0, 1)
        assert float((mine - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
        # the adjoint pair the backward uses: <im2col(x), g> == <x, col2im(g)> on the valid frames
        g = torch.randn(Lx, B, K, generator=R._gen(4)).double()
        colx = C.column_matrix((x.double() * m).float(), torch.tensor(lens), KW).reshape(Lx, B, K)
        dx, _ = E.col2im(g, torch.tensor(lens), Cin, KW)
        lhs, rhs = float((colx * g).sum()), float(((x.double() * m).float().double() * dx).sum())
        assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), 1.0)


def _plan(M, N, K, a_km, b_km, lda, ldb, flags=0, beta=0.0, work=0, bias=False):
    from flowtron_amd import _lib as L
    fake = 4096                                          # the query looks at pointers for NULL and alignment only
    a = L.GemmImgArgs(fake, fake, fake, fake if bias else None, M, N, K, lda, ldb, N, a_km, b_km, 1.0, beta, 0, flags, None, None, 0, 0, None, None,
                      fake if work else None, work, None)
    p = L.GemmImgPlan()
    rc = L.lib().ft_gemm_img_plan(ctypes.byref(a), ctypes.byref(p))
    return rc, p


def test_plan_query_answers_what_the_gpu_file_expects():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    for case, c in G.CASES.items():
        Lx, B, Cin, Cout, KW, rows, K = G.dims(case)
        took = K % 32 == 0 and ops.images_apply(R.BF16, rows, Cout, K)
        assert took == (c["path"] == "split"), case
        if not took:
            assert (K % 32 != 0) != (rows * Cout * K < (1 << 20)), "each fallback case is reached by ONE of the two rules"
            assert ops.images_apply(R.BF16, rows, Cout, K) == (c["bwd"] == "images")
            continue
        need = L.lib().ft_gemm_img_split_work_bytes(rows, Cout, 3 * K)
        ld = C.up(3 * K, 256)
        rc, p = _plan(rows, Cout, 3 * K, 0, 0, ld, ld, flags=L.GEMM_SPLITK_DET if need else 0, work=need, bias=True)
        assert rc == 0
        for k, v in c["fwd"].items():
            got = getattr(p, k)
            assert (v(got) if callable(v) else got == v), (case, k, got)
    assert G.dims("full")[6] * 3 == 7680
