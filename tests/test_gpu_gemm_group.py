"""-m gpu: the grouped weight-gradient GEMMs (ft_gemm_img_group / ft_gemm_img_group_f16: several problems dW = dY^T X, both operand
images k-major, in one grid per tile height) against the float64 restatement of tests/gemm_ref64.py, with the input classes, the
bound and the helpers of tests/test_gpu_gemm_f64.py: on the exact-sum class any association of the sum -- one slice, several slices
combined by atomics, two problems adding into one C -- equals float64 bit for bit; the rounded class stays within that file's bound.
Every C lies in a wider buffer of sentinels that must come back untouched."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import gemm_ref64 as R
from test_gpu_gemm_f64 import FMTS, SENT, alpha_of, dev, env, image_of, judge, sources, up, vector  # noqa: F401  (env: the fixture)

pytestmark = pytest.mark.gpu


def c_buffer(cls, rows, N, seed, c_off=0, ld_pad=5, width=None):
    """(buffer of sentinels, the [rows, N] window at (1, c_off) preloaded with random C0, C0 float64 on the device, ldc)"""
    ldc = up((c_off + N if width is None else width) + ld_pad, 4)
    cbuf = torch.full((rows + 2, ldc), SENT, dtype=torch.float32, device="cuda")
    C0 = vector(cls, rows * N, seed + 7).reshape(rows, N)
    view = cbuf[1:1 + rows, c_off:c_off + N]
    view.copy_(C0.cuda())
    return cbuf, view, C0.cuda().double(), ldc


def problem(env, fmt, cls, M, N, K, seed, *, beta=0.0, want_bias=False, idx=0, splitk=True, target=None, c_off=0, width=None):
    """a plain (compact = 0) weight-gradient problem on fresh k-major images; target = (cbuf, view, C0, ldc) of another problem: the same C"""
    L, ops = env
    a, b = sources(cls, M, K, seed), sources(cls, N, K, seed + 1)
    bias = vector(cls, N, seed + 2) if want_bias else None
    alpha = alpha_of(cls, K, idx)
    if cls == "exact":
        R.assert_exact_case(a, b, alpha, beta, C0=torch.full((1,), 5.0), bias=bias)
    ad, bd = dev(a), dev(b)
    A, B = image_of(ops, ad, 1, fmt), image_of(ops, bd, 1, fmt)
    a64, b64 = R.operands(R.round_op(ad, fmt), R.round_op(bd, fmt), M=M, N=N, K=K)
    cbuf, view, C0, ldc = target if target is not None else c_buffer(cls, M, N, seed, c_off=c_off, width=width)
    kw = dict(bias=dev(bias), alpha=alpha, beta=beta, splitk=splitk)
    args, _ = ops._gemm_img_args(A, 1, A.ptr(), B, 1, B.ptr(), view, M, N, K, ldc, **kw)
    return SimpleNamespace(args=args, keep=(A, B, kw), a64=a64, b64=b64, cbuf=cbuf, view=view, C0=C0, M=M, N=N, K=K, k_len=None, alpha=alpha,
                           beta=beta, bias=kw["bias"], fmt=fmt, cls=cls, c_off=c_off, call=(A, 1, A.ptr(), B, 1, B.ptr(), view, M, N, K, ldc, kw))


def compact_problem(env, fmt, cls, cap, M, N, rows, k_shift, seed, idx=0):
    """compact = 2, beta = 1: k-major images [cap rows][M] / [cap rows][N], zero in rows [rows, rows + 64), DATA beyond that the
    reduction must not reach; *rows_dev = rows"""
    L, ops = env
    d, x = sources(cls, cap, M, seed, specials=False), sources(cls, cap, N, seed + 1, specials=False)
    d[rows:rows + 64] = 0
    x[rows:rows + 64] = 0
    dd, xd = dev(d), dev(x)
    A, B = ops.Bf16Image(dd, mode=fmt), ops.Bf16Image(xd, mode=fmt)
    rm = SimpleNamespace(map=torch.zeros(1, dtype=torch.int32, device="cuda"), rows=torch.tensor([rows], dtype=torch.int32, device="cuda"), cap=cap)
    a64, b64 = R.operands(R.round_op(dd, fmt), R.round_op(xd, fmt), M=M, N=N, K=cap, a_km=True, b_km=True, a_off=(k_shift, 0), compact=2,
                          rows=rows, k_shift=k_shift)
    k_len = max(0, rows - k_shift)
    alpha = alpha_of(cls, max(k_len, 1), idx)
    if cls == "exact" and k_len:
        R.assert_exact_case(d[:rows].t(), x[:rows].t(), alpha, 1.0, C0=torch.full((1,), 5.0))
    cbuf, view, C0, ldc = c_buffer(cls, M, N, seed)
    kw = dict(alpha=alpha, beta=1.0, splitk=True, rowmap=rm, compact=2, k_shift=k_shift)
    args, _ = ops._gemm_img_args(A, 1, A.ptr(k_shift), B, 1, B.ptr(), view, M, N, cap, ldc, **kw)
    return SimpleNamespace(args=args, keep=(A, B, kw), a64=a64, b64=b64, cbuf=cbuf, view=view, C0=C0, M=M, N=N, K=cap, k_len=k_len, alpha=alpha,
                           beta=1.0, bias=None, fmt=fmt, cls=cls, c_off=0)


def run_group(env, probs, fmt):
    L, ops = env
    plans = ops.gemm_img_group_plan([p.args for p in probs])
    ops.gemm_img_group([p.args for p in probs], fmt)
    torch.cuda.synchronize()
    return plans


def untouched_outside(p, tag, others=()):
    guard = p.cbuf.clone()
    for q in (p,) + tuple(others):
        guard[1:1 + q.M, q.c_off:q.c_off + q.N] = SENT
    assert bool((guard == SENT).all()), "%s: wrote outside C" % tag


def check(p, plan, tag):
    untouched_outside(p, tag)
    ref, bound = R.reference(p.a64, p.b64, alpha=p.alpha, beta=p.beta, C0=p.C0, bias=p.bias, k_len=p.k_len, fmt=p.fmt, slices=plan.splits,
                             split=bool(plan.atomics))
    judge(p.cls, p.view.clone(), ref, bound, None, tag)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("cls", ["exact", "rounded"])
def test_five_problems_in_one_call(env, cls, fmt):
    """tall tile with slices, short tile with slices, beta = 1 with a non-zero addend and bias, a column window of a wider matrix
    (ldc > N), and an unsplit problem that leaves through plain stores -- one call, two launches (one per tile height)"""
    probs = [problem(env, fmt, cls, 520, 260, 4160, 11, idx=0),
             problem(env, fmt, cls, 300, 130, 2080, 12, idx=1),
             problem(env, fmt, cls, 260, 130, 2112, 13, beta=1.0, want_bias=True, idx=2),
             problem(env, fmt, cls, 160, 96, 2080, 14, idx=3, c_off=8, width=200),
             problem(env, fmt, cls, 300, 130, 96, 15, idx=0)]
    plans = run_group(env, probs, fmt)
    got = [(p.tile_rows, p.launch) for p in plans]
    assert got == [(256, 0), (128, 1), (128, 1), (128, 1), (128, 1)], got
    assert plans[0].splits >= 2 and plans[0].atomics == 1
    assert all(p.splits > 1 and p.atomics == 1 for p in plans[1:4]), [(p.splits, p.atomics) for p in plans]
    assert plans[4].splits == 1 and plans[4].atomics == 0
    short = sorted(plans[1:], key=lambda p: p.unit0)
    assert short[0].unit0 == 0 and all(a.unit0 + a.tiles * a.splits == b.unit0 for a, b in zip(short, short[1:]))
    assert [p.ksteps for p in short] == sorted((p.ksteps for p in short), reverse=True)
    for i, (p, pl) in enumerate(zip(probs, plans)):
        check(p, pl, "group5 #%d f%d" % (i, fmt))


LENS = tuple(70 - (67 * i) // 31 for i in range(32))             # 70, 68, ..., 3 over B = 32


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("k_shift", [0, 1])
def test_compact_reduction_in_a_group(env, k_shift, fmt):
    """compact = 2: the reduction runs over the rows the batch has (the row map of LENS over T = 70, B = 32: sum + one separator each,
    no multiple of 32) and the kernel divides THOSE over the slices the host chose for the capacity; a batch of 40 rows leaves the last
    slices without rows, a batch of none leaves them all: its C comes back as it was"""
    T, B = 70, 32
    rows = R.row_map_ref(LENS, T, B)[1]
    cap = T * B + B
    assert rows % 32 != 0 and cap >= 2048
    for i, cls in enumerate(("exact", "rounded")):
        probs = [compact_problem(env, fmt, cls, cap, 130, 132, rows, k_shift, 300 + i, idx=i),
                 compact_problem(env, fmt, cls, cap, 520, 130, rows, k_shift, 310 + i, idx=i + 1),      # the tall tile
                 compact_problem(env, fmt, cls, cap, 130, 96, 40, k_shift, 320 + i, idx=i),
                 compact_problem(env, fmt, cls, cap, 96, 130, 0, k_shift, 330 + i, idx=i)]
        plans = run_group(env, probs, fmt)
        assert all(p.splits > 2 for p in plans), [p.splits for p in plans]          # 40 rows = 2 k-steps: slices beyond them are empty
        assert plans[1].tile_rows == 256 and plans[0].tile_rows == 128
        for j, (p, pl) in enumerate(zip(probs, plans)):
            check(p, pl, "compact2 group #%d shift%d f%d %s" % (j, k_shift, fmt, cls))
        assert torch.equal(probs[3].view.double(), probs[3].C0), "a batch without rows changed C"


@pytest.mark.parametrize("fmt", FMTS)
def test_shared_and_disjoint_outputs(env, fmt):
    """two problems adding into the SAME C (beta = 1) sum to both products and are planned atomic although each has one slice; two
    problems on disjoint column windows of one matrix are both plain"""
    for i, cls in enumerate(("exact", "rounded")):
        M, N, K = 200, 130, 96
        p0 = problem(env, fmt, cls, M, N, K, 40 + i, beta=1.0, idx=i, splitk=False)
        p1 = problem(env, fmt, cls, M, N, K, 50 + i, beta=1.0, idx=i + 1, splitk=False, target=(p0.cbuf, p0.view, p0.C0, p0.args.ldc))
        wide = c_buffer(cls, M, 300, 60 + i)
        q0 = problem(env, fmt, cls, M, 130, K, 61 + i, beta=1.0, idx=i, splitk=False, target=(wide[0], wide[1][:, :130], wide[2][:, :130], wide[3]))
        q1 = problem(env, fmt, cls, M, 170, K, 62 + i, beta=0.0, idx=i, splitk=False, target=(wide[0], wide[1][:, 130:], wide[2][:, 130:], wide[3]))
        q1.c_off = 130
        plans = run_group(env, [p0, p1, q0, q1], fmt)
        assert [(p.splits, p.atomics) for p in plans] == [(1, 1), (1, 1), (1, 0), (1, 0)]
        untouched_outside(p0, "shared C")
        r0, b0 = R.reference(p0.a64, p0.b64, alpha=p0.alpha, beta=1.0, C0=p0.C0, fmt=fmt, slices=1, split=True)
        r1, b1 = R.reference(p1.a64, p1.b64, alpha=p1.alpha, beta=1.0, C0=r0, fmt=fmt, slices=1, split=True)
        judge(cls, p0.view.clone(), r1, b0 + b1, None, "shared C f%d" % fmt)
        untouched_outside(q0, "column windows", others=(q1,))
        for q, pl, tag in ((q0, plans[2], "left window"), (q1, plans[3], "right window")):
            ref, bound = R.reference(q.a64, q.b64, alpha=q.alpha, beta=q.beta, C0=q.C0, fmt=fmt, slices=1, split=False)
            judge(cls, q.view.clone(), ref, bound, None, "%s f%d" % (tag, fmt))


@pytest.mark.parametrize("fmt", FMTS)
def test_group_of_one_equals_the_single_call(env, fmt):
    L, ops = env
    for i, cls in enumerate(("exact", "rounded")):
        p = problem(env, fmt, cls, 300, 130, 2080, 70 + i, beta=1.0, want_bias=True, idx=i)
        before = p.view.clone()
        plans = run_group(env, [p], fmt)
        check(p, plans[0], "group of one f%d" % fmt)
        grouped = p.view.clone()
        p.view.copy_(before)
        A, akm, aptr, B, bkm, bptr, view, M, N, K, ldc, kw = p.call
        single = ops.gemm_img_plan(A, akm, aptr, B, bkm, bptr, view, M, N, K, ldc, **kw)
        ops.gemm_img(A, akm, aptr, B, bkm, bptr, view, M, N, K, ldc, **kw)
        torch.cuda.synchronize()
        check(p, single, "the single call f%d" % fmt)
        if cls == "exact":
            assert torch.equal(grouped, p.view)


class ManyWeights(torch.autograd.Function):
    """y = x; the gradient of weight i is one small image GEMM through ops.weight_grad_gemm"""

    @staticmethod
    def forward(ctx, x, ops, jobs, *ws):
        ctx.ops, ctx.jobs = ops, jobs
        ctx.save_for_backward(*ws)
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ops, outs = ctx.ops, []
        for w, (A, B, M, N, K) in zip(ctx.saved_tensors, ctx.jobs):
            dW = torch.zeros_like(w)
            ops.weight_grad_gemm(w, dW, A, A.ptr(), B, B.ptr(), dW, M, N, K, N, beta=1.0)
            outs.append(dW)
        return (g, None, None) + tuple(outs)


@pytest.mark.parametrize("n", [48, 49])
def test_full_table_and_one_more(env, monkeypatch, n):
    """48 problems fill the table of one call; the 49th of a backward pass goes into a second call through the Python flush"""
    L, ops = env
    assert L.GEMM_GROUP_MAX == 48
    fmt, M, N, K = R.BF16, 40, 36, 64
    a, b = sources("exact", M, K, 5), sources("exact", N, K, 6)
    A, B = image_of(ops, dev(a), 1, fmt), image_of(ops, dev(b), 1, fmt)
    want = (R.round_op(dev(a), fmt).double() @ R.round_op(dev(b), fmt).double().t()).float()
    ws = [torch.zeros(M, N, device="cuda", requires_grad=True) for _ in range(n)]
    calls = []
    real = ops.gemm_img_group
    monkeypatch.setattr(ops, "gemm_img_group", lambda args, f, st=None: (calls.append(len(args)), real(args, f, st))[1])
    x = torch.ones(3, device="cuda", requires_grad=True)
    ManyWeights.apply(x, ops, [(A, B, M, N, K)] * n, *ws).sum().backward()
    torch.cuda.synchronize()
    assert calls == ([48] if n == 48 else [48, 1]), calls
    assert not ops._DWQ["items"]
    for w in ws:
        assert torch.equal(w.grad, want)
    # the native call refuses more than its table holds
    args = [ops._gemm_img_args(A, 1, A.ptr(), B, 1, B.ptr(), w.grad, M, N, K, N, beta=1.0, splitk=True)[0] for w in ws] * 2
    arr = (L.GemmImgArgs * 49)(*args[:49])
    assert L.lib().ft_gemm_img_group(arr, 49, L.stream()) != 0
