"""tests/gemm_ref64.py checked on the CPU: the exact class IS exact under every accumulation order and split an fp32 kernel could use,
the rounded class stays within its bound for the same emulated accumulations, every wrong reference is at least SHARP times the bound
away at the shapes where tests/test_gpu_gemm_f64.py claims sharpness, the index restatements agree with hand-written cases, and the
plans that file expects are what ft_gemm_img_plan answers (the query touches no device)."""
import ctypes
import math

import pytest
import torch

import gemm_ref64 as R
import test_gpu_gemm_f64 as G

ORDERS = ("fwd", "rev", "shuffle")
SLICES = (1, 3, 64)


def _exact_inputs(M, N, K, seed):
    a, b = R.exact_matrix(M, K, seed), R.exact_matrix(N, K, seed + 1)
    return a, b, R.exact_matrix(M, N, seed + 2), R.exact_vector(N, seed + 3), R.exact_vector(M, seed + 4), R.exact_vector(N, seed + 5)


@pytest.mark.parametrize("K", G.ALL_K)
def test_exact_class_is_exact_in_any_order_and_split(K):
    """fp32 accumulation in 32-wide chunks, forward / reverse / shuffled, in 1, 3 and 64 slices, then the fp32 epilogue: torch.equal with
    the float64 reference at every (K, alpha, beta) of the GPU file"""
    M, N = 9, 7
    a, b, C0, bias, r1r, r1c = _exact_inputs(M, N, K, K)
    for alpha in G.EXACT_ALPHAS:
        for beta in G.EXACT_BETAS:
            R.assert_exact_case(a, b, alpha, beta, C0=C0, bias=bias, r1_row=r1r, r1_col=r1c)
            ref, _ = R.reference(a.double(), b.double(), alpha=alpha, beta=beta, C0=C0.double(), bias=bias, r1_row=r1r, r1_col=r1c, act=R.ACT_RELU)
            assert torch.equal(ref, ref.float().double()), "the exact value is not an fp32 number"
            for order in ORDERS:
                for sl in SLICES:
                    got = R.emulate_call(a.double(), b.double(), alpha=alpha, beta=beta, C0=C0, bias=bias, r1_row=r1r, r1_col=r1c, order=order,
                                         slices=sl, seed=K, relu=True)
                    assert torch.equal(got, R.exact_round(ref, None)), (K, alpha, beta, order, sl)
    for fmt in (R.BF16, R.F16):                        # 16-bit C: ONE rounding of the exact value
        ref, _ = R.reference(a.double(), b.double(), alpha=0.5, C0=C0.double())
        assert torch.equal(R.exact_round(ref, fmt), R.emulate_call(a.double(), b.double(), alpha=0.5, C0=C0).to(R.op_dtype(fmt)))


def test_exact_class_generator_refuses_an_inexact_case():
    a, b = torch.full((2, 1 << 18), 8.0), torch.full((2, 1 << 18), 8.0)
    with pytest.raises(AssertionError):
        R.assert_exact_case(a, b, 1.0)
    with pytest.raises(AssertionError):
        R.assert_exact_case(a[:, :64], b[:, :64], 0.3)
    R.assert_exact_case(a[:, :(1 << 17)], b[:, :(1 << 17)], 1.0)


@pytest.mark.parametrize("fmt", [R.F32, R.BF16, R.F16])
def test_rounded_class_is_within_its_bound(fmt):
    worst = 0.0
    for K in G.ALL_K:
        M, N = 12, 11
        a, b = R.round_op(R.rounded_matrix(M, K, K, zeros=True), fmt), R.round_op(R.rounded_matrix(N, K, K + 1), fmt)
        C0, bias = torch.randn(M, N, generator=R._gen(K + 2)), torch.randn(N, generator=R._gen(K + 3))
        alpha = 1.0 / math.sqrt(K)
        for sl in SLICES:
            sl_eff = min(sl, -(-K // 32))
            ref, bound = R.reference(a.double(), b.double(), alpha=alpha, beta=0.25, C0=C0.double(), bias=bias, fmt=fmt, slices=sl_eff, split=sl_eff > 1)
            for order in ORDERS:
                got = R.emulate_call(a.double(), b.double(), alpha=alpha, beta=0.25, C0=C0, bias=bias, order=order, slices=sl, seed=K)
                worst = max(worst, R.ratio(got, ref, bound))
    print("rounded class, fmt %d: largest emulated |err| / bound = %.3f" % (fmt, worst))
    assert worst <= 1.0, worst


def test_activation_and_c16_bounds_hold_for_fp32_libm():
    """tanh / sigmoid evaluated in fp32 by the kernels' own expressions (1 - 2 / (exp(2x) + 1), 1 / (1 + exp(-x))), and a 16-bit result"""
    K, M, N = 130, 40, 33
    a, b = R.round_op(R.rounded_matrix(M, K, 1), R.BF16), R.round_op(R.rounded_matrix(N, K, 2), R.BF16)
    alpha = 1.0 / math.sqrt(K)
    pre = R.emulate_call(a.double(), b.double(), alpha=alpha)
    for act, fn in ((R.ACT_TANH, lambda x: 1.0 - 2.0 / (torch.exp(2.0 * x) + 1.0)), (R.ACT_SIGMOID, lambda x: 1.0 / (1.0 + torch.exp(-x))),
                    (R.ACT_RELU, lambda x: x.clamp(min=0))):
        ref, bound = R.reference(a.double(), b.double(), alpha=alpha, act=act)
        r = R.ratio(fn(pre), ref, bound)
        print("act %d: %.3f of the bound" % (act, r))
        assert r <= 1.0
    for fmt in (R.BF16, R.F16):
        a2, b2 = R.round_op(R.rounded_matrix(M, K, 1, specials=False), fmt), R.round_op(R.rounded_matrix(N, K, 2, specials=False), fmt)
        ref, bound = R.reference(a2.double(), b2.double(), alpha=alpha, c16=fmt, fmt=fmt)
        got = R.emulate_call(a2.double(), b2.double(), alpha=alpha).to(R.op_dtype(fmt))
        assert R.ratio(got, ref, bound) <= 1.0
        off = (got.double() + 1.01 * R.ulp16(got.double(), fmt))                       # one 16-bit ulp off must NOT pass
        assert R.ratio(off, ref, bound) > 1.0


# ------------------------------------------------------------------------------------------------------------------ sharpness
def _sharp(got, wrong, bound, what, seen):
    r = R.ratio(got, wrong, bound)
    seen.append((what, r))
    assert r >= R.SHARP, "%s: only %.2f x the bound" % (what, r)


@pytest.mark.parametrize("fmt", [R.BF16, R.F16])
def test_every_wrong_reference_is_sharp_at_the_claimed_shapes(fmt):
    """the emulated kernel passes (ratio <= 1) and each mutation of gemm_ref64.MUTATIONS fails by >= SHARP, at G.SHARP_SHAPES"""
    seen, used = [], set()
    f32 = torch.float32

    # store and atomics: A a column block of a wider source full of +-BIG
    for fam, slices in (("store", 1), ("atomics", 4)):
        M, N, K = G.SHARP_SHAPES[fam]
        assert K <= R.SHARP_MAX_K
        wide = torch.full((M + 3, 8 + K + 8), G.BIG)
        wide[::2] = -G.BIG
        wide[:M, 8:8 + K] = R.rounded_matrix(M, K, 1)
        aw, br = R.round_op(wide, fmt), R.round_op(R.rounded_matrix(N, K, 2), fmt)
        C0, bias = torch.randn(M, N, generator=R._gen(3)), torch.randn(N, generator=R._gen(4))
        kw = dict(alpha=1.0 / math.sqrt(K), beta=1.0 if slices > 1 else 0.25, bias=bias)
        a64, b64 = R.operands(aw, br, M=M, N=N, K=K, a_off=(0, 8))
        got = R.emulate_call(a64, b64, C0=C0, slices=slices, **kw)
        rk = dict(C0=C0.double(), fmt=fmt, slices=slices, split=slices > 1, **kw)
        ref, bound = R.reference(a64, b64, **rk)
        assert R.ratio(got, ref, bound) <= 1.0
        for mut in ("drop_k", "drop_last_step", "swap_groups"):
            am, bm = R.operands(aw, br, M=M, N=N, K=K, a_off=(0, 8), mut=mut, mut_arg=K // 2 + 1)
            _sharp(got, R.reference(am, bm, **rk)[0], bound, "%s %s" % (fam, mut), seen)
        _sharp(got, R.reference(a64, b64, pad_term=R.pad_in_term(aw, (0, 8), M, K, b64), **rk)[0], bound, fam + " pad_in", seen)
        for mut in ("no_beta", "bias_shift"):
            _sharp(got, R.reference(a64, b64, mut=mut, **rk)[0], bound, "%s %s" % (fam, mut), seen)
        used |= {"drop_k", "drop_last_step", "swap_groups", "pad_in", "no_beta", "bias_shift"}

    # compact = 1: row map and the rank-1 term's row
    cap, N, K = G.SHARP_SHAPES["compact1"]
    T, B = 40, 4
    lst, rows = R.row_map_ref([40, 31, 30, 23], T, B)
    assert len(lst) == rows <= cap == T * B + B
    x, w = R.round_op(R.rounded_matrix(T * B, K, 5), fmt), R.round_op(R.rounded_matrix(N, K, 6), fmt)
    a_src = torch.stack([x[r] if r >= 0 else torch.zeros(K) for r in lst])
    a64, b64 = R.operands(a_src, w, M=cap, N=N, K=K)
    C0, r1r, r1c = torch.randn(T * B, N, generator=R._gen(7)), torch.randn(T * B, generator=R._gen(8)), torch.randn(N, generator=R._gen(9))
    kw = dict(alpha=1.0 / math.sqrt(K), beta=0.25, r1_row=r1r, r1_col=r1c, rowmap=lst, rows=rows)
    got = R.emulate_call(a64, b64, C0=C0, **kw)
    ref, bound = R.reference(a64, b64, C0=C0.double(), fmt=fmt, **kw)
    assert R.ratio(got, ref, bound) <= 1.0
    for mut in ("rowmap_shift", "r1_compact_row"):
        wrong, wb = R.reference(a64, b64, C0=C0.double(), fmt=fmt, mut=mut, **kw)
        _sharp(got, wrong, torch.maximum(bound, wb), "compact1 " + mut, seen)
        used.add(mut)

    # compact = 2: the reduction's limit
    M, N, cap = G.SHARP_SHAPES["compact2"]
    rows, k_shift = 98, 1
    d, xx = R.rounded_matrix(cap, M, 10, specials=False), R.rounded_matrix(cap, N, 11, specials=False)
    d[rows:rows + 64] = 0
    xx[rows:rows + 64] = 0
    okw = dict(M=M, N=N, K=cap, a_km=True, b_km=True, a_off=(k_shift, 0), compact=2, rows=rows, k_shift=k_shift)
    a64, b64 = R.operands(R.round_op(d, fmt), R.round_op(xx, fmt), **okw)
    C0 = torch.randn(M, N, generator=R._gen(12))
    kw = dict(alpha=1.0 / math.sqrt(rows), beta=1.0)
    got = R.emulate_call(a64[:, :128], b64[:, :128], C0=C0, slices=4, **kw)            # (the kernel visits the first 4 k-steps only)
    rk = dict(C0=C0.double(), fmt=fmt, slices=8, split=True, k_len=rows - k_shift, **kw)
    ref, bound = R.reference(a64, b64, **rk)
    assert R.ratio(got, ref, bound) <= 1.0
    for mut in ("k_shift_off", "rows_beyond", "drop_k"):
        am, bm = R.operands(R.round_op(d, fmt), R.round_op(xx, fmt), mut=mut, mut_arg=rows // 2 + 1, **okw)
        _sharp(got, R.reference(am, bm, **rk)[0], bound, "compact2 " + mut, seen)
        used.add(mut)

    # row gather
    _, N, K = G.SHARP_SHAPES["gather"]
    T, B, lens = 30, 5, [30, 22, 11, 4, 0]
    whole, wrows = R.row_map_ref(lens, T, B)
    x, w = R.round_op(R.rounded_matrix(T * B, K, 13), fmt), R.round_op(R.rounded_matrix(N, K, 14), fmt)
    img = torch.stack([x[r] if r >= 0 else torch.zeros(K) for r in whole])
    a_rows, rmap, crows = R.chunk_gather_rows_ref(lens, T, B, 10, 20)
    filled = [r if r is not None else 0 for r in a_rows]
    a64, b64 = R.operands(img, w, M=crows, N=N, K=K, a_rows=filled, rows=crows)
    for i, r in enumerate(a_rows):                      # the gathered rows ARE the chunk's frames of x
        if r is not None:
            t, bb = divmod(rmap[i], B)
            assert torch.equal(a64[i].float(), x[(10 + t) * B + bb])
    kw = dict(alpha=1.0 / math.sqrt(K), rowmap=rmap, rows=crows)
    C0 = torch.randn(10 * B, N, generator=R._gen(15))
    got = R.emulate_call(a64, b64, C0=C0, **kw)
    ref, bound = R.reference(a64, b64, C0=C0.double(), fmt=fmt, **kw)
    assert R.ratio(got, ref, bound) <= 1.0
    am, bm = R.operands(img, w, M=crows, N=N, K=K, a_rows=filled, rows=crows, mut="a_rows_shift")
    _sharp(got, R.reference(am, bm, C0=C0.double(), fmt=fmt, **kw)[0], bound, "gather a_rows_shift", seen)
    used.add("a_rows_shift")

    for what, r in seen:
        print("fmt %d  %-28s %10.1f x the bound" % (fmt, what, r))
    assert used == set(R.MUTATIONS), set(R.MUTATIONS) - used


# ------------------------------------------------------------------------------------------------------------------ indexing
def test_row_map_and_chunk_rows_by_hand():
    # T = 3, B = 3, lens (2, 0, 3): utterance 0 = frames (0,0) (1,0) + separator (2,0); 1 = separator (0,1); 2 = three frames, no separator
    assert R.row_map_ref([2, 0, 3], 3, 3) == ([0, 3, 6, 1, 2, 5, 8, -1], 8)
    # chunk [1, 3): lengths (1, 0, 2); image offsets of the utterances 0, 3, 4
    a_rows, rmap, rows = R.chunk_gather_rows_ref([2, 0, 3], 3, 3, 1, 3)
    assert (a_rows, rmap, rows) == ([1, None, None, 5, 6, None], [0, -1, -1, 2, 5, -1], 6)
    whole = R.row_map_ref([2, 0, 3], 3, 3)[0]
    for a, r in zip(a_rows, rmap):                      # image row a_rows[i] holds the frame the chunk writes to its row rmap[i]
        if a is not None:
            t, b = divmod(r, 3)
            assert whole[a] == (1 + t) * 3 + b


def test_operands_by_hand():
    src = torch.arange(24, dtype=torch.float32).reshape(4, 6)                  # image [4 rows][6 cols]
    a, _ = R.operands(src, src, M=2, N=1, K=3, a_off=(1, 2))
    assert a.tolist() == [[8, 9, 10], [14, 15, 16]]
    a, _ = R.operands(src, src, M=3, N=1, K=5, a_off=(2, 3))                   # beyond the source: the image's zero padding
    assert a.tolist() == [[15, 16, 17, 0, 0], [21, 22, 23, 0, 0], [0, 0, 0, 0, 0]]
    a, b = R.operands(src, src, M=3, N=2, K=2, a_km=True, b_km=True, a_off=(1, 0), b_off=(0, 4))     # k-major: rows are k
    assert a.tolist() == [[6, 12], [7, 13], [8, 14]] and b.tolist() == [[4, 10], [5, 11]]
    a, _ = R.operands(src, src, M=3, N=1, K=4, a_km=True, a_off=(1, 0), compact=2, rows=3, k_shift=1)  # k < rows - k_shift = 2
    assert a.tolist() == [[6, 12, 0, 0], [7, 13, 0, 0], [8, 14, 0, 0]]
    a, _ = R.operands(src, src, M=3, N=1, K=2, a_rows=[3, 0, 1], rows=2)
    assert a.tolist() == [[18, 19], [0, 1], [0, 0]]
    ref, bound = R.reference(torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=R.F64), torch.tensor([[1.0, 1.0]], dtype=R.F64), alpha=2.0, beta=0.5,
                             C0=torch.tensor([[4.0], [8.0], [16.0]], dtype=R.F64), bias=torch.tensor([1.0]), r1_row=torch.tensor([1.0, 2.0, 3.0]),
                             r1_col=torch.tensor([10.0]), rowmap=[2, -1], rows=2)
    assert ref.tolist() == [[4.0], [8.0], [2 * 3 + 0.5 * 16 + 1 + 3 * 10]] and bound[:2].abs().sum() == 0 and bound[2, 0] > 0


# ------------------------------------------------------------------------------------------------------------------ the plan query
def _plan(M, N, K, a_km=0, b_km=0, flags=0, beta=0.0, compact=0, a_rows=False, work=0, ldc=None):
    from flowtron_amd import _lib as L
    fake = 4096                                          # the query looks at pointers for NULL and alignment only
    a = L.GemmImgArgs(fake, fake, fake, None, M, N, K, 256, 256, ldc or (N + 3) // 4 * 4, a_km, b_km, 1.0, beta, 0, flags,
                      fake if compact else None, fake if compact else None, compact, 0, None, None, fake if work else None, work,
                      fake if a_rows else None)
    p = L.GemmImgPlan()
    rc = L.lib().ft_gemm_img_plan(ctypes.byref(a), ctypes.byref(p))
    return rc, p


def test_plan_query_answers_what_the_gpu_file_expects():
    from flowtron_amd import _lib as L
    seen = set()
    for name, (M, N, K, split, expect) in G.PATHS.items():
        for a_km, b_km in G.LAYOUTS:
            rc, p = _plan(M, N, K, a_km, b_km, flags=L.GEMM_SPLITK if split else 0)
            assert rc == 0
            want = dict(expect)
            want.setdefault("stage_k", 32 if (a_km and b_km) else 64)
            for k, v in want.items():
                got = getattr(p, k)
                assert (v(got) if callable(v) else got == v), (name, a_km, b_km, k, got)
            seen.add((a_km, b_km, p.tile_rows, p.stage_k, p.gather, p.atomics))
    for b_km in (0, 1):
        rc, p = _plan(55, 131, 192, 0, b_km, compact=1, a_rows=True)
        assert rc == 0 and (p.tile_rows, p.stage_k, p.gather, p.atomics) == (128, 64, 1, 0)
        seen.add((0, b_km, 128, 64, 1, 0))
    assert seen == set(G.INSTANTIATIONS)
    # refused exactly where the call is refused
    assert _plan(55, 131, 96, 0, 0, compact=1, a_rows=True)[0] != 0             # K % 64 != 0
    assert _plan(55, 131, 192, 1, 0, compact=1, a_rows=True)[0] != 0            # k-major A
    assert _plan(130, 132, 96, flags=L.GEMM_C16, beta=1.0)[0] != 0
    assert L.lib().ft_gemm_img_plan(None, None) != 0
    # deterministic split-K: the workspace clips the slices
    need = L.lib().ft_gemm_img_split_work_bytes(96, 36, 2560)
    rc, p = _plan(96, 36, 2560, flags=L.GEMM_SPLITK_DET, work=need)
    assert rc == 0 and p.det == 1 and p.atomics == 0 and p.splits == need // (96 * 36 * 4)
    rc, p = _plan(96, 36, 2560, flags=L.GEMM_SPLITK_DET, work=3 * 96 * 36 * 4 + 8)
    assert rc == 0 and p.det == 1 and 1 < p.splits <= 3
    rc, p = _plan(96, 36, 2560, flags=L.GEMM_SPLITK_DET, work=96 * 36 * 4)
    assert rc == 0 and p.det == 0 and p.splits == 1
