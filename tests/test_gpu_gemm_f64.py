"""Every GEMM kernel path against float64 (-m gpu): ft_gemm_img (csrc/gemm_bf16.hip), the staging ft_gemm (csrc/gemm.hip) and
ft_img_gemv_rows / _bwd, called through ops.gemm_img / ops.gemm_raw, compared element by element with tests/gemm_ref64.py.

Two input classes per case (gemm_ref64's docstring): "exact" -- small integers and powers of two, on which the kernel must equal the
float64 reference BIT FOR BIT (torch.equal; with 16-bit C: equal to its one RNE rounding), atomics included -- and "rounded" -- N(0, 1)
data with the 16-bit formats' edge values planted, held to the derived bound (ratio <= 1, the largest ratio is printed per case).

Every ft_gemm_img case first ASSERTS its plan (ft_gemm_img_plan: the launcher's own decision), so each case knows which instantiation
of gemm_bf16_k it ran; INSTANTIATIONS lists the 21 that launch_s can produce and the last test of the file asserts that the cases,
collected from their asserted plans, covered all of them in both operand formats.  Paths are reached by SHAPE, never by the
library's once-per-process environment hooks.

Sharpness: each family (store, atomics, compact 1, compact 2, gather, staging) is also compared with the wrong references of
gemm_ref64.MUTATIONS under the same bound, and every one must be off by >= SHARP times the bound.  The rounded-class shapes that claim
sharpness for the single-element mutations are SHARP_SHAPES (all K <= gemm_ref64.SHARP_MAX_K = 2048); at longer K the bound is as
large as one product and the exact class carries that duty (one missing product of integers changes an exact result).

Measured on the MI355X (profiles/gemm_f64_pytest_gpu.log holds every printed figure): no kernel failed a case.  Largest rounded-class ratio
with fp32 C 0.24 of the bound; with 16-bit C 0.998 (the half ulp of the one rounding IS the bound's leading term); the closest wrong
reference is 845 times the bound away (atomics, one dropped k of 2048)."""
import ctypes
import math
from types import SimpleNamespace

import pytest
import torch

import gemm_ref64 as R

pytestmark = pytest.mark.gpu

FMTS = (R.BF16, R.F16)
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
SENT = -512.0                                   # sentinel in C's neighbourhood (representable in fp32, bf16 and fp16)
BIG = 3.0e4                                     # neighbour values of operand views: large, finite, representable in both formats

# (a_kmajor, b_kmajor, tile_rows, stage_k, gather, atomics): what launch_s (csrc/gemm_bf16.hip) can instantiate per operand format
INSTANTIATIONS = tuple(
    [(a, b, t, 32, 0, at) for a, b in LAYOUTS for t in (256, 128) for at in (1, 0)]
    + [(a, b, 128, 64, 0, 0) for a, b in LAYOUTS if not (a and b)]
    + [(0, b, 128, 64, 1, 0) for b in (0, 1)])
assert len(INSTANTIATIONS) == 21 and len(set(INSTANTIATIONS)) == 21
COVERED = set()                                 # (fmt,) + instantiation, from the asserted plans of the cases that ran

# rounded-class shapes that claim sharpness for the single-element mutations (family -> (M, N, K)); every reduction <= R.SHARP_MAX_K
# (compact1 / gather: M = the capacity; compact2: K = the capacity 4100, the reduction itself runs over 97 rows)
SHARP_SHAPES = {"store": (130, 131, 100), "atomics": (300, 130, 2048), "compact1": (164, 131, 96), "compact2": (130, 132, 4100),
                "gather": (55, 131, 192), "staging": (130, 131, 130)}


EXACT_ALPHAS = (0.5, -2.0, 0.25, 1.0)               # alpha_of's cycle, and the betas of the exact-class cases
EXACT_BETAS = (0.0, 1.0, 0.25)
# every reduction length of this file (tests/test_gemm_ref64_cpu.py proves the exact class exact and the bound sound at each)
ALL_K = (19, 64, 72, 76, 80, 96, 97, 98, 100, 127, 128, 130, 192, 255, 257, 300, 1023, 1024, 1032, 1376, 1664, 2048, 2050, 2080, 2100, 2112,
         2560, 2592, 5000, 8200)


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.lib()
    return L, ops


def up(v, m):
    return (v + m - 1) // m * m


def dev(t):
    return t.cuda() if t is not None else None


def sources(cls, rows, cols, seed, **kw):
    return R.exact_matrix(rows, cols, seed) if cls == "exact" else R.rounded_matrix(rows, cols, seed, **kw)


def vector(cls, n, seed):
    return R.exact_vector(n, seed) if cls == "exact" else torch.randn(n, generator=R._gen(seed))


def alpha_of(cls, K, i=0):
    return EXACT_ALPHAS[i % 4] if cls == "exact" else 1.0 / math.sqrt(K)


def image_of(ops, src, km, fmt):
    """the operand image of the logical [rows, K] fp32 matrix `src` (device): k-contiguous, or k-major = the image of its transpose"""
    return ops.Bf16Image(src.t().contiguous() if km else src.contiguous(), mode=fmt)


def run_img(env, fmt, cls, A, a_ptr, a_km, B, b_ptr, b_km, a64, b64, M, N, K, *, expect, alpha, beta=0.0, bias=None, act=0, r1=None,
            c16=False, splitk=False, rm=None, rm_list=None, rows=None, compact=0, k_shift=0, a_rows=None, out_rows=None, c_off=0,
            ld_pad=5, nan_c=False, split_work_bytes=None, seed=0, tag="", k_len=None):
    """One ft_gemm_img call: assert its plan, run it into a strided C surrounded by sentinels, return (got, ref, bound, info); info carries
    the plan's splits / atomics / det and C0 (float64, as the reference saw it) for the wrong references of the sensitivity tests.
    k_len: the reduction the kernel walks when it is not K (compact = 2).
    a64 / b64: the dense float64 operands (gemm_ref64.operands).  C0 is random (exact class: integers; nan_c: NaN) also when beta = 0,
    where it must not matter; rows the call does not write must come back as they were."""
    L, ops = env
    assert (K if k_len is None else k_len) in ALL_K, "add this reduction length to ALL_K: the CPU file proves the classes at each"
    out_rows = M if out_rows is None else out_rows
    cdt = ops.op16_dtype(fmt) if c16 else torch.float32
    ldc = up(c_off + N + ld_pad, 4)
    cbuf = torch.full((out_rows + 2, ldc), SENT, dtype=cdt, device="cuda")
    C0 = vector(cls, out_rows * N, seed + 7).reshape(out_rows, N)
    if nan_c:
        C0 = torch.full_like(C0, float("nan"))
    if c16:
        C0 = C0.to(cdt).float()
    view = cbuf[1:1 + out_rows, c_off:c_off + N]
    view.copy_(C0.cuda())
    kw = dict(bias=bias, act=act, alpha=alpha, beta=beta, splitk=splitk, rowmap=rm, compact=compact, k_shift=k_shift, c16=c16, a_rows=a_rows)
    if r1 is not None:
        kw["rank1"] = (r1[0], r1[1].data_ptr())
    if split_work_bytes is not None:
        kw["split_work_bytes"] = split_work_bytes
    plan = ops.gemm_img_plan(A, a_km, a_ptr, B, b_km, b_ptr, view, M, N, K, ldc, **kw)
    inst = (int(a_km), int(b_km), plan.tile_rows, plan.stage_k, plan.gather, plan.atomics)
    for k, v in expect.items():
        got = getattr(plan, k)
        assert (v(got) if callable(v) else got == v), "%s: plan.%s = %d, plan %s" % (tag, k, got, inst + (plan.det, plan.splits, plan.chunk_w))
    assert inst in INSTANTIATIONS, inst
    ops.gemm_img(A, a_km, a_ptr, B, b_km, b_ptr, view, M, N, K, ldc, **kw)
    torch.cuda.synchronize()
    COVERED.add((fmt,) + inst)
    got = view.clone()
    guard = cbuf.clone()
    guard[1:1 + out_rows, c_off:c_off + N] = SENT
    assert bool((guard == SENT).all()), "%s: wrote outside C [%d, %d] (ldc %d)" % (tag, out_rows, N, ldc)
    C0d = C0.cuda().double()
    ref, bound = R.reference(a64, b64, alpha=alpha, beta=beta, C0=C0d, bias=bias, k_len=k_len, r1_row=r1[0] if r1 else None,
                             r1_col=r1[1] if r1 else None, act=act, rowmap=rm_list, rows=rows, c16=fmt if c16 else None, fmt=fmt,
                             slices=plan.splits, split=bool(plan.atomics or plan.det))
    return got, ref, bound, SimpleNamespace(splits=plan.splits, atomics=plan.atomics, det=plan.det, chunk_w=plan.chunk_w, C0=C0d)


def judge(cls, got, ref, bound, c16fmt, tag):
    if cls == "exact":
        want = R.exact_round(ref, c16fmt)
        assert torch.equal(got, want), "%s exact: %d of %d elements differ, max |d| %g" % (
            tag, int((got != want).sum()), got.numel(), float((got.double() - want.double()).abs().max()))
    else:
        r = R.ratio(got, ref, bound)
        print("%s rounded: max |err| / bound = %.3f" % (tag, r))
        assert r <= 1.0, "%s: error %.3f x the bound" % (tag, r)


def plain_case(env, fmt, M, N, K, a_km, b_km, cls, *, expect, idx=0, want_bias=False, beta=0.0, act=0, splitk=False, c16=False,
               c_off=0, nan_c=False, split_work_bytes=None, tag=""):
    """a plain (compact = 0) call on proper images of fresh sources"""
    L, ops = env
    seed = 1000 * idx + 17 * M + 3 * N + K
    a = sources(cls, M, K, seed, specials=not c16)
    b = sources(cls, N, K, seed + 1, specials=not c16)
    bias = vector(cls, N, seed + 2) if want_bias else None
    alpha = alpha_of(cls, K, idx)
    if cls == "exact":
        R.assert_exact_case(a, b, alpha, beta, C0=torch.full((1,), 5.0), bias=bias)
    ad, bd = dev(a), dev(b)
    A, B = image_of(ops, ad, a_km, fmt), image_of(ops, bd, b_km, fmt)
    a64, b64 = R.operands(R.round_op(ad, fmt), R.round_op(bd, fmt), M=M, N=N, K=K)
    got, ref, bound, plan = run_img(env, fmt, cls, A, A.ptr(), a_km, B, B.ptr(), b_km, a64, b64, M, N, K, expect=expect, alpha=alpha,
                                    beta=beta, bias=dev(bias), act=act, splitk=splitk, c16=c16, c_off=c_off, nan_c=nan_c,
                                    split_work_bytes=split_work_bytes, seed=seed, tag=tag)
    judge(cls, got, ref, bound, fmt if c16 else None, tag)
    return got, plan


# ------------------------------------------------------------------------------------------------------------------ the paths
# name -> (M, N, K, split flag, expected plan).  Smallest shapes that reach the path with ragged M, N (no multiples of 128 or 4) and K.
STORE = dict(tile_rows=128, gather=0, atomics=0, det=0, splits=1)
PATHS = {
    "store128_k32":  (130, 131, 96, False, dict(STORE, stage_k=32, chunk_w=0)),
    "store128_k64":  (130, 131, 64, False, dict(STORE, chunk_w=0)),               # stage_k: 64, but 32 for k-major x k-major (asserted below)
    "store128_k100": (130, 131, 100, False, dict(STORE, chunk_w=0)),              # K not a multiple of 32; the last wide stage reaches 28 past K
    "atomics128":    (300, 130, 2080, True, dict(tile_rows=128, stage_k=32, atomics=1, det=0, splits=lambda s: s > 1)),
    "atomics128_e":  (300, 130, 2112, True, dict(tile_rows=128, stage_k=32, atomics=1, det=0, splits=lambda s: s > 1)),   # even k-steps: still 32-wide
    "atomics256":    (520, 1030, 8200, True, dict(tile_rows=256, stage_k=32, atomics=1, det=0, splits=lambda s: s > 1)),
    "store256":      (770, 8200, 2050, True, dict(tile_rows=256, stage_k=32, atomics=0, det=0, splits=1, chunk_w=0)),     # >= 256 tall tiles, un-chunked order
    "store256_l2":   (4090, 2040, 2080, True, dict(tile_rows=256, stage_k=32, atomics=0, det=0, splits=1, chunk_w=lambda w: w > 0)),
    "l2order_k64":   (2050, 130, 64, False, dict(STORE, chunk_w=lambda w: w > 0)),          # gy = 17 (17 % 8 != 0), gx = 2
    "l2order_k96":   (2050, 130, 96, False, dict(STORE, stage_k=32, chunk_w=lambda w: w > 0)),
    "l2order_gx":    (2050, 700, 1376, False, dict(STORE, stage_k=32, chunk_w=lambda w: w > 0)),   # gx = 6 is no multiple of chunk_w = 5
}


BIG_PATHS = ("atomics256", "store256", "store256_l2")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("a_km,b_km", LAYOUTS)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_path_against_float64(env, path, a_km, b_km, fmt):
    M, N, K, split, expect = PATHS[path]
    expect = dict(expect)
    if "stage_k" not in expect:                          # the k-major x k-major layout has no wide form
        expect["stage_k"] = 32 if (a_km and b_km) else 64
    for i, cls in enumerate(("exact", "rounded")):
        if path in BIG_PATHS and cls == "rounded" and (a_km + b_km + fmt) % 2:
            continue                                      # the largest shapes: the exact class everywhere, the rounded one once per layout
        beta = 1.0 if (split and cls == "rounded") else 0.0            # (the atomic paths add into a preloaded C)
        plain_case(env, fmt, M, N, K, a_km, b_km, cls, expect=expect, idx=i + 2 * a_km + b_km, want_bias=True, beta=beta, splitk=split,
                   tag="%s[%d%d f%d]" % (path, a_km, b_km, fmt))


def test_l2_order_chunk_width_is_not_a_divisor_of_gx(env):
    """the l2order_gx shape really has gx % chunk_w != 0 (else the ragged last chunk of the L2-aware order is not reached)"""
    L, ops = env
    M, N, K = PATHS["l2order_gx"][:3]
    A, B = ops.Bf16Image._blank(M, K, R.BF16, "cuda"), ops.Bf16Image._blank(N, K, R.BF16, "cuda")
    c = torch.empty(M, N, device="cuda")
    plan = ops.gemm_img_plan(A, 0, A.ptr(), B, 0, B.ptr(), c, M, N, K, N)
    gx, gy = up(N, 128) // 128, up(M, 128) // 128
    assert plan.chunk_w > 1 and gx % plan.chunk_w != 0 and gy >= 16 and gy % 8 != 0, (plan.chunk_w, gx, gy)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("a_km,b_km", LAYOUTS)
@pytest.mark.parametrize("K", [2560, 2592])
def test_deterministic_split(env, K, a_km, b_km, fmt):
    """FT_GEMM_SPLITK_DET at (96, 36, K), K = 0 and 32 (mod 64): the full workspace and one that holds fewer slices than asked for (`fit`
    clips them) -- two runs of each are bit-identical, and on the exact class both equal the reference"""
    L, ops = env
    M, N = 96, 36
    need = L.lib().ft_gemm_img_split_work_bytes(M, N, K)
    assert need >= 4 * M * N * 4
    wide = 64 if (K % 64 == 0 and not (a_km and b_km)) else 32
    for work, nsl in ((None, need // (M * N * 4)), (3 * M * N * 4 + 8, 3)):
        expect = dict(tile_rows=128, stage_k=wide, atomics=0, det=1, splits=lambda s, n=nsl: 1 < s <= n)
        for i, cls in enumerate(("exact", "rounded")):
            outs = [plain_case(env, fmt, M, N, K, a_km, b_km, cls, expect=expect, idx=i, want_bias=True, splitk="det", split_work_bytes=work,
                               tag="det K%d[%d%d f%d] work=%s" % (K, a_km, b_km, fmt, work))[0] for _ in range(2)]
            assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------------ epilogue
EPI_SHAPES = {64: (130, 131, 64), 96: (130, 131, 96)}
EPILOGUES = {
    "beta0": dict(), "beta0_bias": dict(want_bias=True), "beta1": dict(beta=1.0), "beta1_bias": dict(beta=1.0, want_bias=True),
    "beta_quarter": dict(beta=0.25), "beta_quarter_bias": dict(beta=0.25, want_bias=True),
    "tanh": dict(beta=0.25, want_bias=True, act=R.ACT_TANH), "relu": dict(beta=0.25, want_bias=True, act=R.ACT_RELU),
    "sigmoid": dict(beta=0.25, want_bias=True, act=R.ACT_SIGMOID),
    "nan_c": dict(nan_c=True, want_bias=True),
    "misaligned_c": dict(c_off=1, beta=0.25, want_bias=True),          # C 4 bytes off a 16-byte boundary: the scalar tail everywhere
    "c16": dict(c16=True, want_bias=True), "c16_misaligned": dict(c16=True, c_off=1),
}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", sorted(EPI_SHAPES))
@pytest.mark.parametrize("epi", sorted(EPILOGUES))
def test_epilogue_store_kernels(env, epi, K, fmt):
    """beta in {0, 1, 1/4} x bias, each activation, NaN in C under beta = 0, the scalar tail (N % 4 != 0; C misaligned) and 16-bit C at one
    64-wide and one 32-wide store shape; ldc > N with sentinels around C in every case (run_img)"""
    M, N, _ = EPI_SHAPES[K]
    kw = dict(EPILOGUES[epi])
    expect = dict(STORE, stage_k=64 if K == 64 else 32)
    for i, cls in enumerate(("exact", "rounded")):
        if cls == "exact" and kw.get("act", 0) in (R.ACT_TANH, R.ACT_SIGMOID):
            continue                                      # (the exact class has no transcendental activations)
        plain_case(env, fmt, M, N, K, 0, i, cls, expect=expect, idx=i, tag="%s K%d f%d" % (epi, K, fmt), **kw)
    if epi in ("beta0", "c16"):                          # N % 4 == 0: whole float4 / 8-byte pieces to the last column
        plain_case(env, fmt, M, 132, K, 0, 0, "exact", expect=expect, idx=3, tag="%s N132 K%d f%d" % (epi, K, fmt), **kw)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("path,beta,want_bias", [("atomics128", 0.0, False), ("atomics128", 1.0, True), ("atomics128", 1.0, False),
                                                 ("atomics128", 0.0, True), ("atomics256", 1.0, False)])
def test_epilogue_atomic_kernels(env, path, beta, want_bias, fmt):
    """the atomic split-K epilogue where it is allowed (beta in {0, 1}, bias, no activation): beta = 0 clears exactly C's N columns of
    the strided rows (the sentinels beside them survive), beta = 1 adds into the preloaded C"""
    M, N, K, split, expect = PATHS[path]
    for i, cls in enumerate(("exact", "rounded")):
        plain_case(env, fmt, M, N, K, 1, 1, cls, expect=dict(expect), idx=i, want_bias=want_bias, beta=beta, splitk=True,
                   tag="%s beta%g bias%d f%d" % (path, beta, want_bias, fmt))


# ------------------------------------------------------------------------------------------------------------------ compact = 1
def compact1_setup(env, fmt, cls, lens, T, B, K, N, seed, b_km=0, specials=True):
    """x [T*B, K] time-major -> its compact image over the row map of `lens`; the map is ALSO restated from the header
    (gemm_ref64.row_map_ref) and compared with the device list"""
    L, ops = env
    x, w = sources(cls, T * B, K, seed, specials=specials), sources(cls, N, K, seed + 1, specials=specials)
    lens32 = torch.tensor(lens, dtype=torch.int32, device="cuda")
    rm = ops.row_map(lens32, T, B)
    lst, rows = R.row_map_ref(lens, T, B)
    assert int(rm.rows.item()) == rows and rm.map[:rows].tolist() == lst and rm.cap == T * B + B
    xd, wd = dev(x), dev(w)
    A = ops.Bf16Image(xd, mode=fmt, rowmap=rm)
    Bi = image_of(ops, wd, b_km, fmt)
    xr = R.round_op(xd, fmt)
    idx = torch.tensor([max(r, 0) for r in lst], device="cuda")
    a_src = xr[idx] * torch.tensor([1.0 if r >= 0 else 0.0 for r in lst], device="cuda")[:, None]      # compact order; -1 = a zero row
    return SimpleNamespace(rm=rm, lst=lst, rows=rows, A=A, B=Bi, a_src=a_src, b_src=R.round_op(wd, fmt), x=x, w=w)


COMPACT1_LENS = {                                     # T = 40, B = 4: *rows_dev = sum (len + 1)
    "tile_multiple_128": [40, 31, 30, 23], "tile_plus_one_129": [40, 31, 30, 24], "tile_minus_one_127": [40, 31, 30, 22],
    "separators_minus_one": [40, 40, 40, 40], "short_and_empty": [3, 0, 17, 1],
}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", [64, 96])
@pytest.mark.parametrize("lens", sorted(COMPACT1_LENS))
def test_compact_rows_with_rank1_and_row_map(env, lens, K, fmt):
    """compact = 1: *rows_dev a multiple of the tile, one more, one less; -1 separators; the rank-1 term at the OUTPUT row (!= the compact
    row), bias, beta = 1/4, and 16-bit C through the row map.  Rows the map drops or never reaches keep their values."""
    T, B, N = 40, 4, 131
    for i, cls in enumerate(("exact", "rounded")):
        for c16 in (False, True):
            s = compact1_setup(env, fmt, cls, COMPACT1_LENS[lens], T, B, K, N, seed=50 + K + i, b_km=i, specials=not c16)
            a64, b64 = R.operands(s.a_src, s.b_src, M=s.rm.cap, N=N, K=K)
            bias, r1r, r1c = vector(cls, N, 3), vector(cls, T * B, 4), vector(cls, N, 5)
            alpha = alpha_of(cls, K, i)
            if cls == "exact":
                R.assert_exact_case(s.x, s.w, alpha, 0.25, C0=torch.full((1,), 5.0), bias=bias, r1_row=r1r, r1_col=r1c)
            expect = dict(STORE, stage_k=64 if K == 64 else 32)
            tag = "compact1 %s K%d c16=%d f%d %s" % (lens, K, c16, fmt, cls)
            got, ref, bound, _ = run_img(env, fmt, cls, s.A, s.A.ptr(), 0, s.B, s.B.ptr(), i, a64, b64, s.rm.cap, N, K, expect=expect,
                                         alpha=alpha, beta=0.0 if c16 else 0.25, bias=dev(bias), r1=(dev(r1r), dev(r1c)),
                                         c16=c16, rm=s.rm, rm_list=s.lst, rows=s.rows, compact=1, out_rows=T * B, seed=K, tag=tag)
            judge(cls, got, ref, bound, fmt if c16 else None, tag)


@pytest.mark.parametrize("fmt", FMTS)
def test_compact_rows_zero_rows_and_l2_capacity(env, fmt):
    """*rows_dev = 0 writes nothing; a capacity with gy >= 16 (the host picks the L2-aware order) whose *rows_dev gives gy < 16 (the kernel
    then takes the plain order over the tiles that exist)"""
    L, ops = env
    T, B, K, N = 500, 4, 64, 131
    s = compact1_setup(env, fmt, "exact", [100, 50, 7, 0], T, B, K, N, seed=77)
    a64, b64 = R.operands(s.a_src, s.b_src, M=s.rm.cap, N=N, K=K)
    a64[s.rows:] = 0
    expect = dict(STORE, stage_k=64, chunk_w=lambda w: w > 0)
    assert up(s.rm.cap, 128) // 128 >= 16 > up(s.rows, 128) // 128
    for cls_rows, rows_t in (("some", None), ("zero", 0)):
        rm, rows = s.rm, s.rows
        if rows_t is not None:
            rm = SimpleNamespace(map=s.rm.map, rows=torch.zeros(1, dtype=torch.int32, device="cuda"), cap=s.rm.cap)
            rows = 0
        got, ref, bound, _ = run_img(env, fmt, "exact", s.A, s.A.ptr(), 0, s.B, s.B.ptr(), 0, a64, b64, s.rm.cap, N, K, expect=expect,
                                     alpha=0.5, beta=1.0, rm=rm, rm_list=s.lst, rows=rows, compact=1, out_rows=T * B, seed=5,
                                     tag="compact1 l2cap rows=%s f%d" % (cls_rows, fmt))
        judge("exact", got, ref, bound, None, "compact1 l2cap rows=%s f%d" % (cls_rows, fmt))


# ------------------------------------------------------------------------------------------------------------------ compact = 2
def compact2_setup(env, fmt, cls, cap, M, N, R_rows, seed):
    """k-major images [cap rows][M] and [cap rows][N] whose rows [R, R + 64) are zero (what ft_bf16_image_rows leaves behind the rows a
    batch has) and whose rows beyond that hold DATA the reduction must not reach"""
    L, ops = env
    d, x = sources(cls, cap, M, seed, specials=False), sources(cls, cap, N, seed + 1, specials=False)
    d[R_rows:R_rows + 64] = 0
    x[R_rows:R_rows + 64] = 0
    dd, xd = dev(d), dev(x)
    return SimpleNamespace(A=ops.Bf16Image(dd, mode=fmt), B=ops.Bf16Image(xd, mode=fmt), a_src=R.round_op(dd, fmt), b_src=R.round_op(xd, fmt),
                           rm=SimpleNamespace(map=torch.zeros(1, dtype=torch.int32, device="cuda"),
                                              rows=torch.tensor([R_rows], dtype=torch.int32, device="cuda"), cap=cap), d=d, x=x)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("k_shift", [0, 1])
@pytest.mark.parametrize("rem", [0, 1, 31])
def test_compact_reduction(env, rem, k_shift, fmt):
    """compact = 2 on the 128-row atomic kernel, both operands k-major: *rows_dev - k_shift = 96 + rem (4 k-steps for 8 slices: half the
    slices exit empty), beta = 1 into a preloaded C; rows at or beyond *rows_dev are not reduced"""
    cap, M, N = 4100, 130, 132
    rows = 96 + rem + k_shift
    for i, cls in enumerate(("exact", "rounded")):
        s = compact2_setup(env, fmt, cls, cap, M, N, rows, seed=90 + rem + i)
        a64, b64 = R.operands(s.a_src, s.b_src, M=M, N=N, K=cap, a_km=True, b_km=True, a_off=(k_shift, 0), compact=2, rows=rows, k_shift=k_shift)
        alpha = alpha_of(cls, rows, i)
        if cls == "exact":
            R.assert_exact_case(s.d[:rows].t(), s.x[:rows].t(), alpha, 1.0, C0=torch.full((1,), 5.0))
        expect = dict(tile_rows=128, stage_k=32, atomics=1, det=0, splits=lambda n: n > (rows + 31) // 32)
        got, ref, bound, _ = run_img(env, fmt, cls, s.A, s.A.ptr(k_shift), 1, s.B, s.B.ptr(), 1, a64, b64, M, N, cap, expect=expect, alpha=alpha,
                                     beta=1.0, splitk=True, rm=s.rm, compact=2, k_shift=k_shift, seed=rem, k_len=rows - k_shift,
                                     tag="compact2 rem%d shift%d f%d" % (rem, k_shift, fmt))
        judge(cls, got, ref, bound, None, "compact2 rem%d shift%d f%d %s" % (rem, k_shift, fmt, cls))


@pytest.mark.parametrize("fmt", FMTS)
def test_compact_reduction_tall_tile(env, fmt):
    """compact = 2 on the 256-row atomic kernel (the weight gradients' own form): capacity 8200, 5001 rows, k_shift = 1"""
    cap, M, N, rows = 8200, 520, 1030, 5001
    s = compact2_setup(env, fmt, "exact", cap, M, N, rows, seed=131)
    a64, b64 = R.operands(s.a_src, s.b_src, M=M, N=N, K=cap, a_km=True, b_km=True, a_off=(1, 0), compact=2, rows=rows, k_shift=1)
    R.assert_exact_case(s.d[:rows].t(), s.x[:rows].t(), 0.5, 1.0, C0=torch.full((1,), 5.0))
    expect = dict(tile_rows=256, stage_k=32, atomics=1, det=0, splits=lambda n: n > 1)
    got, ref, bound, _ = run_img(env, fmt, "exact", s.A, s.A.ptr(1), 1, s.B, s.B.ptr(), 1, a64, b64, M, N, cap, expect=expect, alpha=0.5, beta=1.0,
                                 splitk=True, rm=s.rm, compact=2, k_shift=1, seed=9, k_len=rows - 1, tag="compact2 tall f%d" % fmt)
    judge("exact", got, ref, bound, None, "compact2 tall f%d" % fmt)


# ------------------------------------------------------------------------------------------------------------------ row gather
def gather_setup(env, fmt, cls, lens, T, B, K, N, t0, t1, seed, b_km):
    """the whole sequence's batch-major compact image of d [T*B, K], and the row lists of the time chunk [t0, t1) -- from
    ft_chunk_gather_rows AND restated from the header; the two are compared where the chunk keeps the row"""
    L, ops = env
    s = compact1_setup(env, fmt, cls, lens, T, B, K, N, seed, b_km=b_km)
    lens32 = torch.tensor(lens, dtype=torch.int32, device="cuda")
    lk = [max(0, min(n - t0, t1 - t0)) for n in lens]
    cm = ops.RowMap(torch.tensor(lk, dtype=torch.int32, device="cuda"), t1 - t0, B)
    ga = ops.ChunkGather(lens32, cm, T, t0, t1)
    a_rows, rmap, rows = R.chunk_gather_rows_ref(lens, T, B, t0, t1)
    torch.cuda.synchronize()
    assert int(ga.rows.item()) == rows and ga.map[:rows].tolist() == rmap
    dev_rows = ga.a_rows[:rows].tolist()
    assert all(a is None or a == d for a, d in zip(a_rows, dev_rows))
    assert all(0 <= d < s.rows for d in dev_rows), "a dropped row must still read a row of the image"
    s.ga, s.a_rows, s.rmap, s.crows = ga, a_rows, rmap, rows
    return s


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("b_km", [0, 1])
@pytest.mark.parametrize("chunk", ["first", "middle", "last"])
def test_row_gather_against_float64(env, chunk, b_km, fmt):
    """a_rows from ft_chunk_gather_rows for a first, a middle and a last time chunk of a ragged batch, against the float64 product of the
    gathered fp32 rows (not against a pre-gathered image)"""
    T, B, N, K = 30, 5, 131, 192
    lens = [30, 22, 11, 4, 0]
    t0, t1 = {"first": (0, 10), "middle": (10, 20), "last": (20, 30)}[chunk]
    for i, cls in enumerate(("exact", "rounded")):
        s = gather_setup(env, fmt, cls, lens, T, B, K, N, t0, t1, seed=200 + i, b_km=b_km)
        a64, b64 = R.operands(s.a_src, s.b_src, M=s.ga.cap, N=N, K=K, a_rows=s.a_rows, rows=s.crows)
        alpha = alpha_of(cls, K, i)
        if cls == "exact":
            R.assert_exact_case(s.x, s.w, alpha)
        expect = dict(tile_rows=128, stage_k=64, gather=1, atomics=0, det=0, splits=1)
        got, ref, bound, _ = run_img(env, fmt, cls, s.A, s.A.ptr(), 0, s.B, s.B.ptr(), b_km, a64, b64, s.ga.cap, N, K, expect=expect, alpha=alpha,
                                     rm=s.ga, rm_list=s.rmap, rows=s.crows, compact=1, a_rows=s.ga.a_rows, out_rows=(t1 - t0) * B, seed=t0,
                                     tag="gather %s b_km%d f%d" % (chunk, b_km, fmt))
        judge(cls, got, ref, bound, None, "gather %s b_km%d f%d %s" % (chunk, b_km, fmt, cls))


# ------------------------------------------------------------------------------------------------------------------ extent contract
def view_setup(env, fmt, cls, M, K, km, kind, seed):
    """a logical [M, K] operand as a view of a wider / taller image whose other entries are +-BIG: kind "cols" = a column block (offset 8),
    "rows" = a row-shifted view (offset 3).  Returns (image, ptr, the wide source rounded, offset in IMAGE coordinates)."""
    L, ops = env
    core = sources(cls, M, K, seed)
    r_off, c_off = (0, 8) if kind == "cols" else (3, 0)
    # image coordinates: k-contiguous [row][k]; k-major [k][row].  Offsets are applied in image coordinates.
    R_img, C_img = (K, M) if km else (M, K)
    tall = up(r_off + up(R_img, 256) + 64, 256)                        # every row a 256-row tile / a 64-wide last stage may read exists
    wide = torch.full((tall, c_off + up(C_img, 256) + 8), BIG)
    wide[::2] = -BIG
    wide[r_off:r_off + R_img, c_off:c_off + C_img] = core.t() if km else core
    wd = dev(wide)
    img = ops.Bf16Image(wd, mode=fmt)
    assert img.ld >= c_off + up(C_img, 256) and img.rows >= r_off + up(R_img, 256)
    return img, img.ptr(r_off, c_off), R.round_op(wd, fmt), (r_off, c_off), core


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", [64, 96, 100])
@pytest.mark.parametrize("kind", ["cols", "rows"])
@pytest.mark.parametrize("a_km,b_km", LAYOUTS)
def test_extent_contract(env, a_km, b_km, kind, K, fmt):
    """whatever lies beyond the logical extent of an operand view is multiplied by the partner's zero padding (k) or dropped (m, n): A
    as a column block / row-shifted view of an image full of +-3e4, B a proper image -- then the roles swapped.  K = 100: the last wide
    stage reaches 28 columns past K; K = 96: the last 32-wide step ends at K"""
    L, ops = env
    M, N = 130, 131
    expect = dict(STORE, stage_k=32 if (a_km and b_km) or K == 96 else 64)
    for i, cls in enumerate(("exact", "rounded")):
        for view_a in (True, False):
            seed = 300 + K + i
            alpha = alpha_of(cls, K, i)
            if view_a:
                A, a_ptr, a_wide, a_off, a_core = view_setup(env, fmt, cls, M, K, a_km, kind, seed)
                b_core = sources(cls, N, K, seed + 1)
                bd = dev(b_core)
                B = image_of(ops, bd, b_km, fmt)
                b_ptr, b_wide, b_off = B.ptr(), (R.round_op(bd, fmt).t() if b_km else R.round_op(bd, fmt)), (0, 0)
            else:
                B, b_ptr, b_wide, b_off, b_core = view_setup(env, fmt, cls, N, K, b_km, kind, seed)
                a_core = sources(cls, M, K, seed + 1)
                ad = dev(a_core)
                A = image_of(ops, ad, a_km, fmt)
                a_ptr, a_wide, a_off = A.ptr(), (R.round_op(ad, fmt).t() if a_km else R.round_op(ad, fmt)), (0, 0)
            if cls == "exact":
                R.assert_exact_case(a_core, b_core, alpha)
            a64, b64 = R.operands(a_wide, b_wide, M=M, N=N, K=K, a_km=a_km, b_km=b_km, a_off=a_off, b_off=b_off)
            tag = "extent %s view_%s K%d [%d%d f%d]" % (kind, "A" if view_a else "B", K, a_km, b_km, fmt)
            got, ref, bound, _ = run_img(env, fmt, cls, A, a_ptr, a_km, B, b_ptr, b_km, a64, b64, M, N, K, expect=expect, alpha=alpha, seed=seed, tag=tag)
            judge(cls, got, ref, bound, None, tag + " " + cls)


# ------------------------------------------------------------------------------------------------------------------ staging GEMM
def pick_mode(ptr, sr, sk, bs, batch):
    """csrc/gemm.hip's three-line rule: 1 = k contiguous (float4 along k), 2 = rows contiguous (register transpose), 0 = generic"""
    al = ptr % 16 == 0 and (batch <= 1 or bs % 4 == 0)
    if sk == 1 and al and sr % 4 == 0:
        return 1
    if sr == 1 and al and sk % 4 == 0:
        return 2
    return 0


def staged_operand(x, mode, batch=1, odd_batch_stride=False):
    """x [batch, R, K] (CPU) laid out so that pick_mode chooses `mode`; returns (device storage, origin tensor, sr, sk, bs)"""
    nb, Rr, K = x.shape
    if mode == 1:
        ld = up(K, 4) + 4
        per = Rr * ld + (1 if odd_batch_stride else 0)
        buf = torch.zeros(nb * per + 8, device="cuda")
        v = torch.as_strided(buf, (nb, Rr, K), (per, ld, 1))
        sr, sk = ld, 1
    elif mode == 2:
        ld = up(Rr, 4) + 4
        per = K * ld + (1 if odd_batch_stride else 0)
        buf = torch.zeros(nb * per + 8, device="cuda")
        v = torch.as_strided(buf, (nb, Rr, K), (per, 1, ld))
        sr, sk = 1, ld
    else:
        ld = up(K, 4) + 1                              # odd row stride: neither float4 form applies
        per = Rr * ld
        buf = torch.zeros(nb * per + 8, device="cuda")
        v = torch.as_strided(buf, (nb, Rr, K), (per, ld, 1))
        sr, sk = ld, 1
    v.copy_(x.cuda())
    return buf, v, sr, sk, per


def staged_case(env, monkeypatch, mode, cls, M, N, K, am, bm, *, batch=1, odd=False, beta=0.25, act=R.ACT_RELU, splitk=False, images=None,
                idx=0, tag=""):
    L, ops = env
    assert K in ALL_K, "add this reduction length to ALL_K: the CPU file proves the classes at each"
    if images is None:                                        # the staging kernel at every size; else: the library's own rule decides
        monkeypatch.setattr(ops, "_BF16_IMAGES", False)
    seed = 400 + 13 * M + 7 * N + K + idx
    zeros = mode != R.F32
    a = torch.stack([sources(cls, M, K, seed + 10 * b, **({} if cls == "exact" else dict(zeros=zeros))) for b in range(batch)])
    b = torch.stack([sources(cls, N, K, seed + 10 * b + 1, **({} if cls == "exact" else dict(zeros=zeros))) for b in range(batch)])
    bias = vector(cls, N, seed + 2)
    alpha = alpha_of(cls, K, idx)
    abuf, av, sAm, sAk, bsA = staged_operand(a, am, batch, odd)
    bbuf, bv, sBn, sBk, bsB = staged_operand(b, bm, batch, odd)
    got_a, got_b = pick_mode(av.data_ptr(), sAm, sAk, bsA, batch), pick_mode(bv.data_ptr(), sBn, sBk, bsB, batch)
    assert (got_a, got_b) == ((0, 0) if odd else (am, bm)), (got_a, got_b)
    ldc = up(N + 5, 4)
    cbuf = torch.full((batch, M + 2, ldc), SENT, device="cuda")
    C0 = vector(cls, batch * M * N, seed + 3).reshape(batch, M, N)
    view = cbuf[:, 1:1 + M, :N]
    view.copy_(C0.cuda())
    a_args = L.GemmArgs(av.data_ptr(), bv.data_ptr(), view.data_ptr(), None, M, N, K, batch, sAm, sAk, sBk, sBn, ldc, bsA, bsB, (M + 2) * ldc,
                        alpha, beta, act, mode, 0, None, 0)
    took_images = ops._BF16_IMAGES and L.lib().ft_gemm_workspace_bytes(ctypes.byref(a_args)) != 0
    assert took_images == bool(images), (took_images, images)
    ops.gemm_raw(av, bv, view, M, N, K, sAm, sAk, sBk, sBn, ldc, bias=dev(bias), act=act, alpha=alpha, beta=beta, batch=batch, bsA=bsA, bsB=bsB,
                 bsC=(M + 2) * ldc, mode=mode, splitk=splitk)
    torch.cuda.synchronize()
    got = view.clone()
    guard = cbuf.clone()
    guard[:, 1:1 + M, :N] = SENT
    assert bool((guard == SENT).all()), tag
    slices = 1
    if splitk and not took_images:                         # csrc/gemm.hip: 768 / tiles, <= K / 512, <= 64, in whole 32-wide steps
        tiles = (up(M, 128) // 128) * (up(N, 128) // 128)
        s = max(1, min(768 // tiles, K // 512, 64)) if tiles < 512 and K >= 2048 and batch == 1 else 1
        kchunk = up(-(-K // 32), s) // s * 32
        slices = -(-K // kchunk)
        assert slices > 1
    if cls == "exact":
        R.assert_exact_case(a.flatten(0, 1), b.flatten(0, 1), alpha, beta, C0=C0, bias=bias)
    for z in range(batch):
        a64, b64 = R.round_op(av[z], mode).double(), R.round_op(bv[z], mode).double()
        ref, bound = R.reference(a64, b64, alpha=alpha, beta=beta, C0=C0[z].cuda().double(), bias=dev(bias), act=act, fmt=mode, slices=slices,
                                 split=slices > 1)
        judge(cls, got[z], ref, bound, None, "%s z%d" % (tag, z))
    return SimpleNamespace(got=got, a=av, b=bv, bias=dev(bias), C0=C0.cuda().double(), alpha=alpha, beta=beta)


STAGE_MODES = (R.F32, R.BF16, R.F16)


@pytest.mark.parametrize("mode", STAGE_MODES)
@pytest.mark.parametrize("K", [19, 130, 1664])
@pytest.mark.parametrize("am", [0, 1, 2])
@pytest.mark.parametrize("bm", [0, 1, 2])
def test_staging_gemm_layouts(env, monkeypatch, bm, am, K, mode):
    """ft_gemm's 3 x 3 operand layouts in FT_F32, bf16 and fp16; the 16-bit modes against the product of the ROUNDED operands"""
    for i, cls in enumerate(("exact", "rounded")):
        staged_case(env, monkeypatch, mode, cls, 130, 131, K, am, bm, idx=i, act=R.ACT_RELU if cls == "exact" else R.ACT_TANH,
                    tag="staging a%d b%d K%d mode%d %s" % (am, bm, K, mode, cls))


@pytest.mark.parametrize("mode", STAGE_MODES)
def test_staging_gemm_batch_and_thin_shapes(env, monkeypatch, mode):
    """batch = 3 with a batch stride that is no multiple of 4 (forces the generic layout on operands that would otherwise vectorise);
    M = 1 and N = 1"""
    for i, cls in enumerate(("exact", "rounded")):
        for am, bm in ((1, 2), (2, 1)):
            staged_case(env, monkeypatch, mode, cls, 65, 7, 130, am, bm, batch=3, odd=True, idx=i, tag="staging batch3 odd a%d b%d mode%d %s" % (am, bm, mode, cls))
            staged_case(env, monkeypatch, mode, cls, 65, 7, 130, am, bm, batch=3, idx=i, tag="staging batch3 a%d b%d mode%d %s" % (am, bm, mode, cls))
        staged_case(env, monkeypatch, mode, cls, 1, 300, 80, 1, 2, idx=i, tag="staging M1 mode%d %s" % (mode, cls))
        staged_case(env, monkeypatch, mode, cls, 513, 1, 1664, 2, 1, idx=i, tag="staging N1 mode%d %s" % (mode, cls))


@pytest.mark.parametrize("mode", STAGE_MODES)
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_staging_gemm_split_k(env, monkeypatch, beta, mode):
    """atomic split-K of the staging kernel at K >= 2048 into a strided C (beta = 0 clears exactly C's columns)"""
    for i, cls in enumerate(("exact", "rounded")):
        staged_case(env, monkeypatch, mode, cls, 130, 131, 2100, 2, 2, beta=beta, act=R.ACT_NONE, splitk=True, idx=i,
                    tag="staging splitk beta%g mode%d %s" % (beta, mode, cls))


@pytest.mark.parametrize("mode", [R.BF16, R.F16])
@pytest.mark.parametrize("M,N,K,images", [(32, 128, 257, True), (32, 128, 255, False), (31, 128, 300, False), (32, 32, 1024, True), (32, 32, 1023, False)])
def test_gemm_image_path_edges(env, monkeypatch, M, N, K, images, mode):
    """ft_gemm's image path through `work` at the edges of its rule (M N K just above / below 2^20, M = 32 versus 31); which path ran is
    asserted through ft_gemm_workspace_bytes"""
    for i, cls in enumerate(("exact", "rounded")):
        staged_case(env, monkeypatch, mode, cls, M, N, K, 1, 2, images=images, idx=i, tag="ft_gemm work (%d,%d,%d) mode%d %s" % (M, N, K, mode, cls))


# ------------------------------------------------------------------------------------------------------------------ N = 1 projections
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", [72, 76, 1032])
def test_image_gemv_rows_and_backward(env, K, fmt):
    """ft_img_gemv_rows / _bwd over a compact image: K % 8 in {0, 4}, *rows_dev no multiple of the backward's 256 rows per block, a padded
    frame receiving its separator's value, db = NULL, accumulation into a preloaded dw"""
    L, ops = env
    T, B = 90, 4
    lens = [90, 61, 88, 30]                                # 273 compact rows: one full block of 256 and 17 more
    for i, cls in enumerate(("exact", "rounded")):
        s = compact1_setup(env, fmt, cls, lens, T, B, K, 8, seed=500 + K + i)
        assert s.rows % 256 not in (0,) and s.rows > 256
        w, bias = vector(cls, K, 11), vector(cls, 1, 12)
        y0 = vector(cls, T * B, 13)
        y, wd, bd = dev(y0.clone()), dev(w), dev(bias)
        L.check(L.op16("ft_img_gemv_rows", fmt)(s.A.buf.data_ptr(), s.A.ld, K, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), 1, s.rm.map.data_ptr(),
                                                s.rm.rows.data_ptr(), s.rm.lens.data_ptr(), T, B, L.stream()), "ft_img_gemv_rows")
        torch.cuda.synchronize()
        ref, bound = R.gemv_rows_ref(s.a_src.cpu(), w, float(bias), s.lst, s.rows, lens, T, B, y0, fmt)
        assert float(ref[(lens[3] + 5) * B + 3]) == float(ref[lens[3] * B + 3]) != float(y0[(lens[3] + 5) * B + 3])     # a padded frame got the separator's value
        judge(cls, y.cpu(), ref, bound, None, "gemv rows K%d f%d %s" % (K, fmt, cls))
        dy = vector(cls, T * B, 14)
        dyd = dev(dy)
        for with_db in (True, False):
            dw0, db0 = vector(cls, K, 15), vector(cls, 1, 16)
            dw, db = dev(dw0.clone()), dev(db0.clone())
            L.check(L.op16("ft_img_gemv_rows_bwd", fmt)(s.A.buf.data_ptr(), s.A.ld, K, dyd.data_ptr(), 1, dw.data_ptr(), db.data_ptr() if with_db else None,
                                                        s.rm.map.data_ptr(), s.rm.rows.data_ptr(), s.rm.cap, L.stream()), "ft_img_gemv_rows_bwd")
            torch.cuda.synchronize()
            rdw, bdw, rdb, bdb = R.gemv_rows_bwd_ref(s.a_src.cpu(), dy, s.lst, s.rows, dw0, float(db0))
            judge(cls, dw.cpu(), rdw, bdw, None, "gemv bwd dw K%d db=%d f%d %s" % (K, with_db, fmt, cls))
            if with_db:
                judge(cls, db.cpu(), torch.tensor([rdb], dtype=R.F64), torch.tensor([bdb], dtype=R.F64), None, "gemv bwd db K%d f%d %s" % (K, fmt, cls))
            else:
                assert torch.equal(db.cpu(), db0)


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def must_be_sharp(got, wrong_ref, bound, what):
    r = R.ratio(got, wrong_ref, bound)
    print("sharp %s: %.1f x the bound" % (what, r))
    assert r >= R.SHARP, "%s is only %.2f x the bound away: the check would not see it" % (what, r)


@pytest.mark.parametrize("fmt", FMTS)
def test_sensitivity_store_and_atomics(env, fmt):
    """the kernel's own output against each applicable wrong reference, under the bound of the right one"""
    L, ops = env
    for fam in ("store", "atomics"):
        M, N, K = SHARP_SHAPES[fam]
        assert K <= R.SHARP_MAX_K
        split = fam == "atomics"
        beta = 1.0 if split else 0.25
        A, a_ptr, a_wide, a_off, _ = view_setup(env, fmt, "rounded", M, K, 0, "cols", 600)
        b = dev(sources("rounded", N, K, 601))
        B = image_of(ops, b, 1, fmt)
        bias = dev(vector("rounded", N, 602))
        alpha = 1.0 / math.sqrt(K)
        br = R.round_op(b, fmt)
        a64, b64 = R.operands(a_wide, br, M=M, N=N, K=K, a_off=a_off)
        expect = dict(tile_rows=128, atomics=int(split), det=0)
        got, ref, bound, info = run_img(env, fmt, "rounded", A, a_ptr, 0, B, B.ptr(), 1, a64, b64, M, N, K, expect=expect, alpha=alpha, beta=beta,
                                        bias=bias, splitk=split, seed=603, tag="sharp " + fam)
        judge("rounded", got, ref, bound, None, "sharp %s f%d" % (fam, fmt))
        common = dict(alpha=alpha, beta=beta, C0=info.C0, bias=bias, fmt=fmt, slices=info.splits, split=split)
        for mut in ("drop_k", "drop_last_step", "swap_groups"):
            am, bm = R.operands(a_wide, br, M=M, N=N, K=K, a_off=a_off, mut=mut, mut_arg=K // 2 + 1)
            must_be_sharp(got, R.reference(am, bm, **common)[0], bound, "%s %s f%d" % (fam, mut, fmt))
        must_be_sharp(got, R.reference(a64, b64, pad_term=R.pad_in_term(a_wide, a_off, M, K, b64), **common)[0], bound, "%s pad_in f%d" % (fam, fmt))
        for mut in ("no_beta", "bias_shift"):
            must_be_sharp(got, R.reference(a64, b64, mut=mut, **common)[0], bound, "%s %s f%d" % (fam, mut, fmt))


@pytest.mark.parametrize("fmt", FMTS)
def test_sensitivity_compact_and_gather(env, fmt):
    L, ops = env
    # compact = 1: the row map, and the rank-1 term's row
    T, B = 40, 4
    _, N, K = SHARP_SHAPES["compact1"]
    s = compact1_setup(env, fmt, "rounded", [40, 31, 30, 23], T, B, K, N, seed=610)
    assert s.rm.cap == SHARP_SHAPES["compact1"][0]
    a64, b64 = R.operands(s.a_src, s.b_src, M=s.rm.cap, N=N, K=K)
    a64[s.rows:] = 0
    r1 = (dev(vector("rounded", T * B, 611)), dev(vector("rounded", N, 612)))
    alpha = 1.0 / math.sqrt(K)
    got, ref, bound, info = run_img(env, fmt, "rounded", s.A, s.A.ptr(), 0, s.B, s.B.ptr(), 0, a64, b64, s.rm.cap, N, K, expect=dict(STORE, stage_k=32),
                                    alpha=alpha, beta=0.25, r1=r1, rm=s.rm, rm_list=s.lst, rows=s.rows, compact=1, out_rows=T * B, seed=613, tag="sharp compact1")
    judge("rounded", got, ref, bound, None, "sharp compact1 f%d" % fmt)
    common = dict(alpha=alpha, beta=0.25, C0=info.C0, r1_row=r1[0], r1_col=r1[1], rowmap=s.lst, rows=s.rows, fmt=fmt)
    for mut in ("rowmap_shift", "r1_compact_row"):
        wrong, wb = R.reference(a64, b64, mut=mut, **common)
        must_be_sharp(got, wrong, torch.maximum(bound, wb), "compact1 %s f%d" % (mut, fmt))
    am, bm = R.operands(s.a_src, s.b_src, M=s.rm.cap, N=N, K=K, mut="drop_k", mut_arg=K // 2 + 1)
    am[s.rows:] = 0
    must_be_sharp(got, R.reference(am, bm, **common)[0], bound, "compact1 drop_k f%d" % fmt)

    # compact = 2: the reduction's limit
    M2, N2, cap = SHARP_SHAPES["compact2"]
    rows, k_shift = 98, 1
    c = compact2_setup(env, fmt, "rounded", cap, M2, N2, rows, seed=620)
    ops_kw = dict(M=M2, N=N2, K=cap, a_km=True, b_km=True, a_off=(k_shift, 0), compact=2, rows=rows, k_shift=k_shift)
    a64, b64 = R.operands(c.a_src, c.b_src, **ops_kw)
    alpha = 1.0 / math.sqrt(rows)
    got, ref, bound, info = run_img(env, fmt, "rounded", c.A, c.A.ptr(k_shift), 1, c.B, c.B.ptr(), 1, a64, b64, M2, N2, cap,
                                    expect=dict(tile_rows=128, stage_k=32, atomics=1), alpha=alpha, beta=1.0, splitk=True, rm=c.rm, compact=2,
                                    k_shift=k_shift, seed=621, k_len=rows - k_shift, tag="sharp compact2")
    judge("rounded", got, ref, bound, None, "sharp compact2 f%d" % fmt)
    common = dict(alpha=alpha, beta=1.0, C0=info.C0, fmt=fmt, slices=info.splits, split=True, k_len=rows - k_shift)
    for mut in ("k_shift_off", "rows_beyond", "drop_k"):
        am, bm = R.operands(c.a_src, c.b_src, mut=mut, mut_arg=rows // 2 + 1, **ops_kw)
        must_be_sharp(got, R.reference(am, bm, **common)[0], bound, "compact2 %s f%d" % (mut, fmt))

    # row gather: the list's entries
    T, B = 30, 5
    _, N, K = SHARP_SHAPES["gather"]
    g = gather_setup(env, fmt, "rounded", [30, 22, 11, 4, 0], T, B, K, N, 10, 20, seed=630, b_km=0)
    a64, b64 = R.operands(g.a_src, g.b_src, M=g.ga.cap, N=N, K=K, a_rows=g.a_rows, rows=g.crows)
    alpha = 1.0 / math.sqrt(K)
    got, ref, bound, info = run_img(env, fmt, "rounded", g.A, g.A.ptr(), 0, g.B, g.B.ptr(), 0, a64, b64, g.ga.cap, N, K,
                                 expect=dict(tile_rows=128, stage_k=64, gather=1), alpha=alpha, rm=g.ga, rm_list=g.rmap, rows=g.crows, compact=1,
                                 a_rows=g.ga.a_rows, out_rows=10 * B, seed=631, tag="sharp gather")
    judge("rounded", got, ref, bound, None, "sharp gather f%d" % fmt)
    common = dict(alpha=alpha, C0=info.C0, rowmap=g.rmap, rows=g.crows, fmt=fmt)
    filled = [a if a is not None else 0 for a in g.a_rows]
    for mut in ("a_rows_shift", "drop_k"):
        am, bm = R.operands(g.a_src, g.b_src, M=g.ga.cap, N=N, K=K, a_rows=filled, rows=g.crows, mut=mut, mut_arg=K // 2 + 1)
        must_be_sharp(got, R.reference(am, bm, **common)[0], bound, "gather %s f%d" % (mut, fmt))


@pytest.mark.parametrize("mode", STAGE_MODES)
def test_sensitivity_staging(env, monkeypatch, mode):
    L, ops = env
    M, N, K = SHARP_SHAPES["staging"]
    c = staged_case(env, monkeypatch, mode, "rounded", M, N, K, 1, 2, idx=0, act=R.ACT_NONE, tag="sharp staging mode%d" % mode)
    got = c.got[0]                                        # the wrong references are built from the case's OWN inputs
    ar, br = R.round_op(c.a[0], mode), R.round_op(c.b[0], mode)
    common = dict(alpha=c.alpha, beta=c.beta, C0=c.C0[0], bias=c.bias, fmt=mode)
    a64, b64 = R.operands(ar, br, M=M, N=N, K=K)
    ref, bound = R.reference(a64, b64, **common)
    assert R.ratio(got, ref, bound) <= 1.0
    for mut in ("drop_k", "drop_last_step", "swap_groups"):
        am, bm = R.operands(ar, br, M=M, N=N, K=K, mut=mut, mut_arg=K // 2 + 1)
        must_be_sharp(got, R.reference(am, bm, **common)[0], bound, "staging %s mode%d" % (mut, mode))
    for mut in ("no_beta", "bias_shift"):
        must_be_sharp(got, R.reference(a64, b64, mut=mut, **common)[0], bound, "staging %s mode%d" % (mut, mode))


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_all_21_instantiations_were_run_in_both_formats():
    """LAST in the file: the plans asserted by the cases above cover every instantiation launch_s can produce, in bf16 and fp16.  It reads
    what the cases of THIS run recorded, so it passes only when the whole file runs in order (a -k selection cannot cover 21 paths, and
    that is what it would say); tests/test_gemm_ref64_cpu.py asserts the same coverage of the case TABLE through the plan query alone."""
    print("%-6s %-6s %-5s %-6s %-6s %-7s  bf16 fp16" % ("a_km", "b_km", "tile", "stage", "gather", "atomics"))
    missing = []
    for inst in INSTANTIATIONS:
        have = [(f,) + inst in COVERED for f in FMTS]
        print("%-6d %-6d %-5d %-6d %-6d %-7d  %-4s %-4s" % (inst + tuple("yes" if h else "NO" for h in have)))
        missing += [(f,) + inst for f, h in zip(FMTS, have) if not h]
    assert not missing, missing
