"""The elementwise, gather, norm, loss and optimizer entry points (csrc/elementwise.hip, csrc/instnorm.hip) against float64 on every path
(-m gpu), called through flowtron_amd._lib's C entry points -- no autograd wrapper in between -- and compared element by element with
tests/elementwise_ref64.py.  Every output buffer is NaN before the call, so a kernel that writes only part of its output fails.

Two input classes (elementwise_ref64's docstring): "exact" -- integers, keep in {0, 2}, targets in {0, 1} -- on which the reductions must
equal the float64 reference BIT FOR BIT, float atomics included, and "bounded" -- N(0, 1)-scaled data under the derived bound (ratio <= 1;
the largest ratio is printed per check and kept in RATIOS).  Pure copies are compared with torch.equal.

Paths are reached by SHAPE and ALIGNMENT:
  * instance norm: C % 4 == 0 and 16-byte aligned pointers -> the float4 pair (16 row lanes x 16 channel quads per 64-channel slab),
    otherwise the scalar pair (4 row lanes x 64 channels); INORM_LENS makes row lanes take 1, 2 and 3 trips, INORM_C makes second slabs and
    slabs partly past C;
  * grid-stride kernels: the PASS2 cases are a little larger than the launch's thread count (the cap of grid_for times 256 threads, written
    next to each case with the line of csrc/elementwise.hip it was read from), and their last elements are valid and checked;
  * ft_embedding_bwd_runs: dim < 128 -> 64-thread blocks, dim >= 128 -> 128-thread blocks (dim 130: blockIdx.y = 1).

The case lists and input builders below are module-level and need no GPU: tests/test_elementwise_ref64_cpu.py iterates the same shapes to
prove the exact class exact, the bound sound under emulated fp32 orders, and every wrong reference of elementwise_ref64.MUTATIONS caught.

Measured on the MI355X (profiles/elementwise_f64_pytest_gpu.log holds every printed figure): no kernel failed a case; 144 tests in 4.2 s.
Largest |err| / bound per entry point: instnorm fwd 0.24, bwd 0.17; affine fwd 0.49, bwd 0.49, inv 0.20; masked_sum 0.002, its bwd 0.37;
gate BCE fwd 0.003, bwd 0.27; fused loss fwd 0.15, bwd 0.41; embedding_bwd 0.07, _runs 0.25; col2im 0.31; colsum 0.02; act_bwd 0.47;
radam 0.50; beta-binomial prior 0.997 (its bound IS the half ulp of the one fp32 rounding).  Every exact-class and copy check: 0 elements
differ."""
import ctypes

import pytest
import torch

import elementwise_ref64 as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
RATIOS = {}                                     # entry point -> largest |err| / bound seen

# ---- launch sizes (threads = grid cap x 256), read from csrc/elementwise.hip
THREADS_DEFAULT = 4096 * 256                    # grid_for(n, per_block = NT, cap = 256 * 16), elementwise.hip:22
THREADS_SUMS = 1024 * 256                       # ft_masked_sum: grid_for(.., NT, 1024), elementwise.hip:610; nll_sums_k: elementwise.hip:646
THREADS_BCE = 256 * 256                         # gate_bce_fwd_k: grid_for(.., NT, 256), elementwise.hip:625 and :649
THREADS_RADAM = 4096 * 256                      # ft_radam_step: grid_for(n, NT, 4096), elementwise.hip:723

# ---- instance norm
INORM_L, INORM_B = 37, 7
INORM_LENS = (37, 42, 33, 17, 16, 5, 1)         # == L, > L (clamped), 2 trips + remainder, 1 trip + 1 row, 1 trip, part of the lanes, 1 frame
INORM_LENS_ZERO = (37, 0, 33, 17, 16, 5, 1)     # one empty sample
INORM_C_Q4 = (4, 64, 68, 132)                   # float4 pair: one quad, one full slab, slab + one quad, two slabs + one quad
INORM_C_SCALAR = (3, 67)                        # scalar pair (C % 4 != 0)
INORM_EPS = 1e-5
# (C, keep, misaligned, lens, class)
INORM_CASES = ([(C, k, False, INORM_LENS, "bounded") for C in INORM_C_Q4 + INORM_C_SCALAR for k in (False, True)]
               + [(68, True, True, INORM_LENS, "bounded")]                                   # C % 4 == 0 on the scalar pair: x one float into a buffer
               + [(68, True, False, INORM_LENS, "exact"), (67, True, False, INORM_LENS, "exact")]
               + [(68, True, False, INORM_LENS_ZERO, "bounded"), (67, False, False, INORM_LENS_ZERO, "bounded")])

# ---- second grid-stride pass: totals a little past the thread count
PASS2_AFFINE = (13108, 80)                      # n_rows, M: 1 048 640 elements
PASS2_IM2COL = (41, 8, 640, 5)                  # L, B, C, KW: 1 049 600 column elements
PASS2_COL2IM = (41, 8, 3200, 3)                 # L B C = 1 049 600 outputs
PASS2_REVERSE = (41, 8, 3200)                   # T, B, C
PASS2_TBM = (164, 80, 80)                       # ft_masked_sum_bwd, nll_bwd_k: 1 049 600
PASS2_FLAT = 1048579                            # ft_act_bwd, ft_eltwise, ft_radam_step
PASS2_EMB = (8195, 128, 50)                     # n, dim, vocab: 1 048 960
PASS2_PRIOR = (9, 400, 292)                     # B, T, L: 1 051 200
PASS2_SUMS = (103, 32, 80)                      # T, B, M: 263 680 > THREADS_SUMS, exact class
PASS2_BCE = (2049, 32)                          # T, B: 65 568 > THREADS_BCE

# ---- small odd shapes
AFFINE_CASES = [(39, M, ext, dx) for M in (1, 3, 80) for ext, dx in ((True, True), (False, False), (True, False))]       # n_rows, M, dls_ext, dx
MSUM_CASES = [(13, 5, 7, 14, (13, 0, 1, 6, 12)), (9, 3, 80, 160, (9, 1, 0))]                                            # T, B, M, ld, lens
BCE_CASES = [(13, 5, (13, 0, 1, 6, 12)), (40, 3, (40, 17, 39))]                                                         # T, B (T != B), lens
BCE_SPECIAL = (0.0, 30.0, -30.0, 100.0, -100.0)
LOSS_CASES = [(11, 4, 5, n_ls, gate, dls, (11, 14, 0, 6)) for n_ls, gate, dls in ((0, True, False), (1, False, True), (8, True, True))]   # one length > T
LOSS_SIGMA = 0.7
EMB_CASES = [(203, dim, dim + pad, 11) for dim, pad in ((1, 0), (64, 3), (65, 0), (128, 4), (130, 0))]                    # n, dim, ld, vocab
RUNS_CASES = [(per * stride - short, dim, stride, ids) for per in (31, 32, 33, 65) for stride, short in ((1, 0), (5, 2))
              for dim in (65, 130) for ids in ("period", "any")]                                                           # n, dim, stride, ids
IM2COL_CASES = [(9, 3, C, KW, (9, 1, 4)) for C in (3, 33) for KW in (1, 3, 5)]                                           # L, B, C, KW, lens
COLSUM_CASES = [(rows, N, N + pad) for N, pad in ((1, 0), (37, 3), (64, 0), (65, 7), (130, 0)) for rows in (0, 1, 31, 33, 1000)]
PADFILL_CASES = [(6, 3, cols, cols + pad, mode, (0, 5, 6)) for cols, pad in ((5, 0), (1024, 4), (1500, 0)) for mode in (0, 1)]    # T, B, cols, ld, mode, lens
REVERSE_CASES = [(7, 4, 5, tm, (7, 0, 1, 4)) for tm in (1, 0)]
ACT_N, ELT_N = 3001, 3001
RADAM_SMALL = 100003
RADAM_HP = dict(clip=1.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step_size=7.3e-4)


# ------------------------------------------------------------------------------------------------------------ input builders (CPU, fp32)
def inorm_inputs(C, keep, lens, cls, seed=0):
    L, B = INORM_L, INORM_B
    if cls == "exact":
        x, dy = R.ints((L, B, C), seed + 1), R.ints((L, B, C), seed + 2)
        gamma, beta = R.ints((C,), seed + 3, 2), R.ints((C,), seed + 4, 2)
    else:
        x, dy = R.normal((L, B, C), seed + 1, 1.5) + 0.5, R.normal((L, B, C), seed + 2)
        gamma, beta = R.normal((C,), seed + 3), R.normal((C,), seed + 4, 0.5)
        x[:, :, 0] = 3.0                                             # a channel constant over time: var = 0, rstd = eps^-1/2
        if C > 1:
            gamma[1] = 0.0
    k = 2.0 * (torch.rand(L, B, C, generator=R.gen(seed + 5)) < 0.7).float() if keep else None
    return x, gamma, beta, k, torch.tensor(lens, dtype=torch.int32), dy


def affine_inputs(n_rows, M, seed=0):
    out = R.normal((n_rows, 2 * M), seed + 1)
    out[:, :M] = out[:, :M].clamp(-3, 3)
    out[0, 0], out[-1, M - 1] = 3.0, -3.0
    return out, R.normal((n_rows, M), seed + 2), R.normal((n_rows, M), seed + 3), R.normal((n_rows, M), seed + 4)    # out, x, dz, dls_ext


def msum_inputs(T, B, M, ld, cls, seed=0):
    return R.ints((T * B, ld), seed + 1) if cls == "exact" else R.normal((T * B, ld), seed + 1)


def bce_inputs(T, B, cls, seed=0):
    gate = R.ints((T, B), seed + 1, 3) if cls == "exact" else R.normal((T, B), seed + 1, 2.0)
    target = (torch.rand(B, T, generator=R.gen(seed + 2)) < 0.3).float()
    if cls != "exact":
        gate[-1] = 30.0 * (1 - 2 * target[:, -1])                    # the last frame (the second pass of PASS2_BCE) carries weight: every term 30
        gate.view(-1)[:len(BCE_SPECIAL)] = torch.tensor(BCE_SPECIAL)
    return gate, target


def loss_inputs(T, B, M, n_ls, cls, seed=0):
    mk = (lambda s, sc=1.0: R.ints(s, seed + 1)) if cls == "exact" else (lambda s, sc=1.0: R.normal(s, seed + 1, sc))
    z = mk((T, B, M))
    lsbuf = [R.ints((T, B, 2 * M), seed + 10 + f) if cls == "exact" else R.normal((T, B, 2 * M), seed + 10 + f, 0.3) for f in range(n_ls)]
    gate, target = bce_inputs(T, B, "bounded", seed + 30)
    return z, lsbuf, gate, target


def runs_ids(n, stride, kind, vocab, seed=0):
    if kind == "period":                                             # ids repeat along the stride: id = speaker of utterance r % stride
        return torch.randint(0, vocab, (stride,), generator=R.gen(seed)).repeat(-(-n // stride))[:n]
    return torch.randint(0, vocab, (n,), generator=R.gen(seed))


def radam_inputs(n, seed=0):
    p, g = R.normal((n,), seed + 1), R.normal((n,), seed + 2, 0.1)
    m, v = R.normal((n,), seed + 3, 0.05), R.normal((n,), seed + 4, 0.01) ** 2
    return p, g, m, v


def full_lens(T, B, seed):
    """lengths in [0, T] with the first and the last sample full: the elements of the second grid-stride pass are the END of the tensor --
    the last frame, of the last samples of the batch -- and some of them are then valid (the CPU file checks that dropping them is seen)"""
    l = torch.randint(0, T + 1, (B,), generator=R.gen(seed), dtype=torch.int32)
    l[0] = l[-1] = T
    return l


# ------------------------------------------------------------------------------------------------------------ GPU helpers
@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.lib()
    return L


def call(L, name, *args):
    L.check(getattr(L.lib(), name)(*args, L.stream()), name)
    torch.cuda.synchronize()


def nanbuf(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def cu(t):
    return None if t is None else t.cuda()


def bounded(name, got, rb, tag=""):
    ref, bound = rb
    r = R.ratio(got, ref, bound)
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    print("%-24s %-40s |err| / bound = %.4f" % (name, tag, r))
    assert r <= 1.0, "%s %s: |err| / bound = %.4f" % (name, tag, r)


def equal(name, got, ref, tag=""):
    ref = torch.as_tensor(ref, dtype=F64).to(got.device).to(torch.float32).reshape(got.shape)
    bad = int((got != ref).sum()) + int(torch.isnan(got).sum())
    print("%-24s %-40s equal: %d of %d differ" % (name, tag, bad, got.numel()))
    assert torch.equal(got, ref), "%s %s: %d of %d elements differ from the float64 reference" % (name, tag, bad, got.numel())


def offset_view(t, off=1):
    """a copy of t that starts `off` floats into a larger buffer (address = 4 * off mod 16)"""
    buf = torch.full((t.numel() + 8,), NAN, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------------------------------ instance norm
@pytest.mark.parametrize("C,keep,misaligned,lens,cls", INORM_CASES)
def test_instnorm(env, C, keep, misaligned, lens, cls):
    L = env
    Ln, B = INORM_L, INORM_B
    x, gamma, beta, k, l32, dy = inorm_inputs(C, keep, lens, cls)
    tag = "C %d keep %d %s %s%s" % (C, keep, "scalar" if (C % 4 or misaligned) else "float4", cls, " len0" if 0 in lens else "")
    fw = R.instnorm_fwd(x, gamma, beta, k, l32, INORM_EPS)
    xd = offset_view(x.cuda()) if misaligned else x.cuda()
    assert (xd.data_ptr() % 16 == 4) == misaligned
    gd, bd, kd, ld_, dyd = cu(gamma), cu(beta), cu(k), cu(l32), cu(dy)
    y, mean, rstd = nanbuf(Ln, B, C), nanbuf(B, C), nanbuf(B, C)
    call(L, "ft_instnorm_relu_fwd", L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(kd), L.ptr(ld_), L.ptr(y), L.ptr(mean), L.ptr(rstd),
         Ln, B, C, INORM_EPS)
    live = torch.tensor([n > 0 for n in lens])
    n = l32.clamp(max=Ln).long()
    pad = (torch.arange(Ln)[:, None] >= n[None, :])
    assert bool((y.cpu()[pad] == 0).all()), tag + ": y must be exactly 0 at l >= len"
    bounded("ft_instnorm_relu_fwd", y, fw["y"], tag + " y")
    bounded("ft_instnorm_relu_fwd", mean.cpu()[live], (fw["mean"][0][live], fw["mean"][1][live]), tag + " mean")
    bounded("ft_instnorm_relu_fwd", rstd.cpu()[live], (fw["rstd"][0][live], fw["rstd"][1][live]), tag + " rstd")
    if cls == "exact":                                               # integer data, power-of-two length: the mean is exact
        p2 = torch.tensor([n_ in (1, 2, 4, 8, 16, 32) for n_ in lens])
        assert int(p2.sum()) >= 2
        R.assert_exact(x.abs().sum(0).max(), 1.0 / 32, x)
        equal("ft_instnorm_relu_fwd", mean[p2.cuda()], fw["mean"][0][p2], tag + " mean (2^k frames)")
    # backward with ITS documented inputs: the y, mean, rstd of the float64 forward, rounded to fp32
    y32, m32, r32 = (fw[q][0].float() for q in ("y", "mean", "rstd"))
    bw = R.instnorm_bwd(x, y32, dy, gamma, k, l32, m32, r32)
    dx = nanbuf(Ln, B, C)
    dgamma, dbeta = torch.full((C,), 1e30, device="cuda"), torch.full((C,), -1e30, device="cuda")      # garbage: the call overwrites them
    y32d, m32d, r32d = cu(y32), cu(m32), cu(r32)
    m32d[~live.cuda()] = NAN                                         # an empty sample's statistics are not defined (the forward leaves 0 / 0 there):
    r32d[~live.cuda()] = NAN                                         # the backward, their only reader, must not let them reach any output
    call(L, "ft_instnorm_relu_bwd", L.ptr(xd), L.ptr(y32d), L.ptr(dyd), L.ptr(gd), L.ptr(kd), L.ptr(ld_), L.ptr(m32d), L.ptr(r32d),
         L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta), Ln, B, C)
    assert bool((dx.cpu()[pad] == 0).all()), tag + ": dx must be exactly 0 at l >= len"
    assert bool(torch.isfinite(dgamma).all()) and bool(torch.isfinite(dbeta).all())
    bounded("ft_instnorm_relu_bwd", dx, bw["dx"], tag + " dx")
    bounded("ft_instnorm_relu_bwd", dgamma, bw["dgamma"], tag + " dgamma")
    bounded("ft_instnorm_relu_bwd", dbeta, bw["dbeta"], tag + " dbeta")
    if cls == "exact":
        R.assert_exact(2 * dy.abs().sum((0, 1)).max(), 1.0, dy)
        equal("ft_instnorm_relu_bwd", dbeta, bw["dbeta"][0], tag + " dbeta (integers)")


# ------------------------------------------------------------------------------------------------------------ coupling
def run_affine(L, n_rows, M, ext, with_dx, tag):
    out, x, dz, dls = affine_inputs(n_rows, M)
    od, xd, dzd, dlsd = cu(out), cu(x), cu(dz), cu(dls) if ext else None
    z = nanbuf(n_rows, M)
    call(L, "ft_affine_fwd", L.ptr(od), L.ptr(xd), L.ptr(z), n_rows, M)
    bounded("ft_affine_fwd", z, R.affine_fwd(od, xd), tag)
    dout, dx = nanbuf(n_rows, 2 * M), nanbuf(n_rows, M) if with_dx else None
    call(L, "ft_affine_bwd", L.ptr(od), L.ptr(xd), L.ptr(dzd), L.ptr(dlsd), L.ptr(dout), L.ptr(dx), n_rows, M)
    bw = R.affine_bwd(od, xd, dzd, dlsd)
    bounded("ft_affine_bwd", dout, bw["dout"], tag + " dout")
    if with_dx:
        bounded("ft_affine_bwd", dx, bw["dx"], tag + " dx")
    xi = nanbuf(n_rows, M)
    call(L, "ft_affine_inv", L.ptr(od), L.ptr(dzd), L.ptr(xi), n_rows, M)              # any z: dz serves
    bounded("ft_affine_inv", xi, R.affine_inv(od, dzd), tag)


@pytest.mark.parametrize("n_rows,M,ext,with_dx", AFFINE_CASES)
def test_affine_small(env, n_rows, M, ext, with_dx):
    run_affine(env, n_rows, M, ext, with_dx, "rows %d M %d ext %d dx %d" % (n_rows, M, ext, with_dx))


def test_affine_second_pass(env):
    n_rows, M = PASS2_AFFINE
    assert n_rows * M > THREADS_DEFAULT
    run_affine(env, n_rows, M, True, True, "pass 2: rows %d M %d" % (n_rows, M))


# ------------------------------------------------------------------------------------------------------------ masked sums
def run_masked_sum(L, T, B, M, ld, lens, cls, tag):
    buf = cu(msum_inputs(T, B, M, ld, cls))
    l32 = cu(torch.as_tensor(lens, dtype=torch.int32))
    for square in (0, 1):
        acc = torch.zeros(1, device="cuda")
        call(L, "ft_masked_sum", L.ptr(buf), ld, L.ptr(l32), L.ptr(acc), square, T, B, M)
        ref, bound = R.masked_sum(buf, M, l32, square, T, B)
        if cls == "exact":
            R.assert_exact((buf[:, :M].double() ** (2 if square else 1)).abs().sum(), 1.0, buf)
            equal("ft_masked_sum", acc, ref, tag + " square %d" % square)
        else:
            bounded("ft_masked_sum", acc, (ref, bound), tag + " square %d" % square)


def run_masked_sum_bwd(L, T, B, M, ld, lens, tag):
    buf = cu(msum_inputs(T, B, M, ld, "bounded"))
    l32 = cu(torch.as_tensor(lens, dtype=torch.int32))
    scale = torch.tensor([0.37], device="cuda")
    for square in (0, 1):
        dxb = nanbuf(T * B, M + 3)
        call(L, "ft_masked_sum_bwd", L.ptr(buf), ld, L.ptr(l32), L.ptr(scale), -1.7, square, L.ptr(dxb), M + 3, T, B, M)
        bounded("ft_masked_sum_bwd", dxb[:, :M], R.masked_sum_bwd(buf, M, l32, float(scale), float(torch.tensor(-1.7, dtype=torch.float32)), square, T, B),
                tag + " square %d" % square)
        assert bool(torch.isnan(dxb[:, M:]).all()), "columns beyond M of a strided dx must stay untouched"


@pytest.mark.parametrize("T,B,M,ld,lens", MSUM_CASES)
@pytest.mark.parametrize("cls", ("exact", "bounded"))
def test_masked_sum_small(env, T, B, M, ld, lens, cls):
    tag = "T %d B %d M %d ld %d %s" % (T, B, M, ld, cls)
    run_masked_sum(env, T, B, M, ld, lens, cls, tag)
    if cls == "bounded":
        run_masked_sum_bwd(env, T, B, M, ld, lens, tag)


def test_masked_sum_second_pass_exact(env):
    T, B, M = PASS2_SUMS
    assert T * B * M > THREADS_SUMS
    run_masked_sum(env, T, B, M, 2 * M, full_lens(T, B, 5), "exact", "pass 2: T %d B %d M %d ld %d" % (T, B, M, 2 * M))


def test_masked_sum_bwd_second_pass(env):
    T, B, M = PASS2_TBM
    assert T * B * M > THREADS_DEFAULT
    run_masked_sum_bwd(env, T, B, M, M, full_lens(T, B, 6), "pass 2: T %d B %d M %d" % (T, B, M))


# ------------------------------------------------------------------------------------------------------------ gate BCE
def bce_depth(total, threads):
    """additions a term of the grid-stride sum passes through: its thread's passes, 6 + 4 of the 256-thread workgroup sum, the atomics"""
    return -(-total // threads) + 10 + threads // 256


def run_bce(L, T, B, lens, tag, depth=None):
    gate, target = bce_inputs(T, B, "bounded")
    gd, td, l32 = cu(gate), cu(target), cu(torch.as_tensor(lens, dtype=torch.int32))
    acc = torch.zeros(1, device="cuda")
    call(L, "ft_gate_bce_fwd", L.ptr(gd), L.ptr(td), L.ptr(l32), L.ptr(acc), T, B)
    bounded("ft_gate_bce_fwd", acc, R.gate_bce_fwd(gd, td, l32, depth=depth), tag)
    scale = torch.tensor([0.37], device="cuda")
    dg = nanbuf(T, B)
    call(L, "ft_gate_bce_bwd", L.ptr(gd), L.ptr(td), L.ptr(l32), L.ptr(scale), -1.7, L.ptr(dg), T, B)
    rb = R.gate_bce_bwd(gd, td, l32, float(scale), float(torch.tensor(-1.7, dtype=torch.float32)))
    bounded("ft_gate_bce_bwd", dg, rb, tag)                           # every frame: valid ones under the bound, padded ones exactly 0 (bound 0)


@pytest.mark.parametrize("T,B,lens", BCE_CASES)
def test_gate_bce_small(env, T, B, lens):
    run_bce(env, T, B, lens, "T %d B %d" % (T, B))


def test_gate_bce_second_pass(env):
    T, B = PASS2_BCE
    assert T * B > THREADS_BCE
    run_bce(env, T, B, full_lens(T, B, 7), "pass 2: T %d B %d" % (T, B), depth=bce_depth(T * B, THREADS_BCE))


# ------------------------------------------------------------------------------------------------------------ fused loss
def run_loss(L, T, B, M, n_ls, with_gate, with_dls, lens, cls, tag):
    z, lsbuf, gate, target = loss_inputs(T, B, M, n_ls, cls)
    zd, gd, td = cu(z), cu(gate) if with_gate else None, cu(target) if with_gate else None
    lsd = [cu(b) for b in lsbuf]
    views = [b[..., :M] for b in lsd]                                 # log_s = the first half of a [T, B, 2M] coupling output: ld = 2M
    l32 = cu(torch.as_tensor(lens, dtype=torch.int32))
    arr = (ctypes.c_void_p * 8)(*[v.data_ptr() for v in views])
    acc, nll, go = nanbuf(8), nanbuf(1), nanbuf(1) if with_gate else None
    call(L, "ft_flowtron_loss_fwd", L.ptr(zd), ctypes.cast(arr, ctypes.c_void_p) if n_ls else None, n_ls, 2 * M, L.ptr(gd), L.ptr(td),
         L.ptr(l32), LOSS_SIGMA, L.ptr(acc), L.ptr(nll), L.ptr(go), T, B, M)
    fw = R.flowtron_loss_fwd(zd, views, gd, td, l32, LOSS_SIGMA)
    name = "ft_flowtron_loss_fwd"
    if cls == "exact":
        R.assert_exact((zd.double() ** 2).sum() + sum(v.double().abs().sum() for v in views), 1.0, zd, *lsd)
        equal(name, acc[0], fw["acc0"][0], tag + " acc[0]")
        equal(name, acc[1], fw["acc1"][0], tag + " acc[1]")
    else:
        bounded(name, acc[0], fw["acc0"], tag + " acc[0]")
        bounded(name, acc[1], fw["acc1"], tag + " acc[1]")
    equal(name, acc[6], fw["acc6"][0], tag + " acc[6] = n")
    bounded(name, acc[4], fw["acc4"], tag + " acc[4] = 1 / (n M)")
    bounded(name, acc[5], fw["acc5"], tag + " acc[5] = 1 / n")
    bounded(name, nll, fw["nll"], tag + " nll")
    if with_gate:
        bounded(name, acc[2], fw["acc2"], tag + " acc[2]")
        bounded(name, go, fw["gate"], tag + " gate loss")
    # backward with its documented inputs: acc as the float64 forward leaves it, rounded to fp32
    accr = torch.zeros(8)
    accr[4], accr[5], accr[6] = float(fw["acc4"][0]), float(fw["acc5"][0]), float(fw["acc6"][0])
    accd = accr.cuda()
    g_nll, g_gate = torch.tensor([1.3], device="cuda"), torch.tensor([-0.6], device="cuda") if with_gate else None
    dz, dls, dgate = nanbuf(T, B, M), nanbuf(T, B, M) if with_dls else None, nanbuf(T, B) if with_gate else None
    call(L, "ft_flowtron_loss_bwd", L.ptr(zd), L.ptr(gd), L.ptr(td), L.ptr(l32), LOSS_SIGMA, L.ptr(accd), L.ptr(g_nll), L.ptr(g_gate),
         L.ptr(dz), L.ptr(dls), L.ptr(dgate), T, B, M)
    bw = R.flowtron_loss_bwd(zd, gd, td, l32, LOSS_SIGMA, float(accr[4]), float(accr[5]), float(g_nll), float(g_gate) if with_gate else None,
                             with_dls=with_dls)
    name = "ft_flowtron_loss_bwd"
    bounded(name, dz, bw["dz"], tag + " dz")
    if with_dls:
        bounded(name, dls, bw["dls"], tag + " dls")
    if with_gate:
        bounded(name, dgate, bw["dgate"], tag + " dgate")


@pytest.mark.parametrize("T,B,M,n_ls,with_gate,with_dls,lens", LOSS_CASES)
@pytest.mark.parametrize("cls", ("exact", "bounded"))
def test_flowtron_loss_small(env, T, B, M, n_ls, with_gate, with_dls, lens, cls):
    """one length is beyond T: n counts it as T, like the masked sums do (header; loss_finalize_k clamps)"""
    run_loss(env, T, B, M, n_ls, with_gate, with_dls, lens, cls, "T %d B %d M %d n_ls %d gate %d %s" % (T, B, M, n_ls, with_gate, cls))


def test_flowtron_loss_fwd_second_pass_exact(env):
    T, B, M = PASS2_SUMS
    assert T * B * M > THREADS_SUMS
    run_loss(env, T, B, M, 2, True, True, full_lens(T, B, 8), "exact", "pass 2: T %d B %d M %d n_ls 2" % (T, B, M))


def test_flowtron_loss_bwd_second_pass(env):
    T, B, M = PASS2_TBM
    assert T * B * M > THREADS_DEFAULT
    run_loss(env, T, B, M, 1, True, True, full_lens(T, B, 9), "bounded", "pass 2: T %d B %d M %d" % (T, B, M))


# ------------------------------------------------------------------------------------------------------------ embedding
def run_embedding(L, n, dim, ld, vocab, tag):
    ids = torch.randint(0, vocab, (n,), generator=R.gen(3)).cuda()
    W = cu(R.normal((vocab, dim), 4))
    out = nanbuf(n, ld)
    call(L, "ft_embedding_fwd", L.ptr(ids), L.ptr(W), L.ptr(out), n, dim, ld)
    equal("ft_embedding_fwd", out[:, :dim].contiguous(), R.embedding_fwd(ids, W)[0], tag)
    assert bool(torch.isnan(out[:, dim:]).all())
    for cls in ("exact", "bounded"):
        dob = cu(R.ints((n, ld), 5) if cls == "exact" else R.normal((n, ld), 5))
        dW = torch.zeros(vocab, dim, device="cuda")
        call(L, "ft_embedding_bwd", L.ptr(ids), L.ptr(dob), L.ptr(dW), n, dim, ld)
        ref, bound = R.embedding_bwd(ids, dob[:, :dim], vocab)
        if cls == "exact":
            R.assert_exact(dob.abs().sum(0).max(), 1.0, dob)
            equal("ft_embedding_bwd", dW, ref, tag + " exact")
        else:
            bounded("ft_embedding_bwd", dW, (ref, bound), tag)


@pytest.mark.parametrize("n,dim,ld,vocab", EMB_CASES)
def test_embedding_small(env, n, dim, ld, vocab):
    run_embedding(env, n, dim, ld, vocab, "n %d dim %d ld %d" % (n, dim, ld))


def test_embedding_second_pass(env):
    n, dim, vocab = PASS2_EMB
    assert n * dim > THREADS_DEFAULT
    run_embedding(env, n, dim, dim, vocab, "pass 2: n %d dim %d" % (n, dim))


@pytest.mark.parametrize("n,dim,stride,kind", RUNS_CASES)
def test_embedding_bwd_runs(env, n, dim, stride, kind):
    """rows per sequence 31 | 32 | 33 | 65 around the 32-row chunk; n not a multiple of the stride; dim 65: 64-thread blocks and a second
    block column, dim 130: 128-thread blocks and a second block column"""
    L = env
    vocab, ld = 7, dim + 2
    ids = runs_ids(n, stride, kind, vocab).cuda()
    tag = "n %d dim %d stride %d ids %s (%d-thread blocks)" % (n, dim, stride, kind, 128 if dim >= 128 else 64)
    for cls in ("exact", "bounded"):
        dob = cu(R.ints((n, ld), 6) if cls == "exact" else R.normal((n, ld), 6))
        dW = torch.zeros(vocab, dim, device="cuda")
        call(L, "ft_embedding_bwd_runs", L.ptr(ids), L.ptr(dob), L.ptr(dW), n, dim, ld, stride)
        ref, bound = R.embedding_bwd(ids, dob[:, :dim], vocab, stride=stride)
        if cls == "exact":
            R.assert_exact(dob.abs().sum(0).max(), 1.0, dob)
            equal("ft_embedding_bwd_runs", dW, ref, tag + " exact")
        else:
            bounded("ft_embedding_bwd_runs", dW, (ref, bound), tag)


# ------------------------------------------------------------------------------------------------------------ im2col / col2im / reverse
def conv_x(Ln, B, C, lens, seed=0):
    """x zero at l >= lens[b], as ft_im2col requires"""
    x = R.normal((Ln, B, C), seed + 1)
    l32 = torch.as_tensor(lens, dtype=torch.int32)
    return x * R.frame_mask(l32, Ln)[:, :, None], l32


def run_im2col(L, Ln, B, C, KW, lens, tag):
    x, l32 = conv_x(Ln, B, C, lens)
    xd, ld_ = cu(x), cu(l32)
    col = nanbuf(Ln, B, C * KW)
    call(L, "ft_im2col", L.ptr(xd), L.ptr(col), L.ptr(ld_), Ln, B, C, KW)
    equal("ft_im2col", col, R.im2col(xd, ld_, KW)[0], tag)


def run_col2im(L, Ln, B, C, KW, lens, tag):
    l32 = cu(torch.as_tensor(lens, dtype=torch.int32))
    for cls in ("exact", "bounded"):
        dcol = cu(R.ints((Ln, B, C * KW), 2) if cls == "exact" else R.normal((Ln, B, C * KW), 2))
        dx = nanbuf(Ln, B, C)
        call(L, "ft_col2im", L.ptr(dcol), L.ptr(dx), L.ptr(l32), Ln, B, C, KW)
        ref, bound = R.col2im(dcol, l32, C, KW)
        if cls == "exact":
            R.assert_exact(KW * dcol.abs().max(), 1.0, dcol)
            equal("ft_col2im", dx, ref, tag + " exact")
        else:
            bounded("ft_col2im", dx, (ref, bound), tag)


@pytest.mark.parametrize("Ln,B,C,KW,lens", IM2COL_CASES)
def test_im2col_col2im_small(env, Ln, B, C, KW, lens):
    tag = "L %d B %d C %d KW %d" % (Ln, B, C, KW)
    run_im2col(env, Ln, B, C, KW, lens, tag)
    run_col2im(env, Ln, B, C, KW, lens, tag)


def test_im2col_second_pass(env):
    Ln, B, C, KW = PASS2_IM2COL
    assert Ln * B * C * KW > THREADS_DEFAULT
    run_im2col(env, Ln, B, C, KW, full_lens(Ln, B, 10), "pass 2: L %d B %d C %d KW %d" % (Ln, B, C, KW))


def test_col2im_second_pass(env):
    Ln, B, C, KW = PASS2_COL2IM
    assert Ln * B * C > THREADS_DEFAULT
    run_col2im(env, Ln, B, C, KW, full_lens(Ln, B, 11), "pass 2: L %d B %d C %d KW %d" % (Ln, B, C, KW))


def run_reverse(L, T, B, C, tm, lens, tag):
    x = cu(R.normal((T, B, C) if tm else (B, T, C), 1))
    l32 = cu(torch.as_tensor(lens, dtype=torch.int32))
    assert int(l32.max()) <= T and int(l32.min()) >= 0
    y = nanbuf(*x.shape)
    call(L, "ft_reverse_by_length", L.ptr(x), L.ptr(y), L.ptr(l32), T, B, C, tm)
    equal("ft_reverse_by_length", y, R.reverse_by_length(x, l32, tm)[0], tag)


@pytest.mark.parametrize("T,B,C,tm,lens", REVERSE_CASES)
def test_reverse_small(env, T, B, C, tm, lens):
    run_reverse(env, T, B, C, tm, lens, "T %d B %d C %d time_major %d" % (T, B, C, tm))


@pytest.mark.parametrize("tm", (1, 0))
def test_reverse_second_pass(env, tm):
    T, B, C = PASS2_REVERSE
    assert T * B * C > THREADS_DEFAULT
    run_reverse(env, T, B, C, tm, full_lens(T, B, 12), "pass 2: T %d B %d C %d time_major %d" % (T, B, C, tm))


# ------------------------------------------------------------------------------------------------------------ colsum, pad fill
@pytest.mark.parametrize("rows,N,ld", COLSUM_CASES)
def test_colsum(env, rows, N, ld):
    L = env
    tag = "rows %d N %d ld %d" % (rows, N, ld)
    for cls in ("exact", "bounded"):
        buf = cu(R.ints((max(rows, 1), ld), 1) if cls == "exact" else R.normal((max(rows, 1), ld), 1))
        out = nanbuf(N + 1)
        call(L, "ft_colsum", L.ptr(buf), L.ptr(out), rows, N, ld)
        ref, bound = R.colsum(buf[:rows, :N])
        assert bool(torch.isnan(out[N:]).all())
        if cls == "exact":
            R.assert_exact(buf.abs().sum(0).max(), 1.0, buf)
            equal("ft_colsum", out[:N], ref, tag + " exact")
        else:
            bounded("ft_colsum", out[:N], (ref, bound), tag)


@pytest.mark.parametrize("T,B,cols,ld,mode,lens", PADFILL_CASES)
def test_pad_rows_fill(env, T, B, cols, ld, mode, lens):
    """lengths 0, T - 1 and T; cols 1500: grid.y = 4 (cols > 1024, elementwise.hip:754)"""
    L = env
    buf = cu(R.normal((T * B, ld), 1))
    before = buf.clone()
    l32 = cu(torch.tensor(lens, dtype=torch.int32))
    call(L, "ft_pad_rows_fill", L.ptr(buf), ld, cols, L.ptr(l32), T, B, mode)
    equal("ft_pad_rows_fill", buf[:, :cols].contiguous(), R.pad_rows_fill(before[:, :cols], l32, T, B, mode)[0],
          "T %d B %d cols %d ld %d mode %d" % (T, B, cols, ld, mode))
    assert torch.equal(buf[:, cols:], before[:, cols:]), "columns beyond cols must stay untouched"


# ------------------------------------------------------------------------------------------------------------ act_bwd, eltwise
def act_inputs(n, act, seed=0):
    """the saved y = act(pre) of a float64 forward, rounded to fp32: the ReLU mask is part of the input"""
    pre = R.normal((n,), seed + 1, 2.0).double()
    y = {R.ACT_NONE: pre, R.ACT_TANH: torch.tanh(pre), R.ACT_RELU: pre.clamp(min=0), R.ACT_SIGMOID: torch.sigmoid(pre)}[act].float()
    return y, R.normal((n,), seed + 2)


@pytest.mark.parametrize("n", (ACT_N, PASS2_FLAT))
@pytest.mark.parametrize("act", (R.ACT_NONE, R.ACT_TANH, R.ACT_RELU, R.ACT_SIGMOID))
def test_act_bwd(env, n, act):
    L = env
    y, dy = act_inputs(n, act)
    yd, dyd, out = cu(y), cu(dy), nanbuf(n)
    call(L, "ft_act_bwd", L.ptr(yd), L.ptr(dyd), L.ptr(out), n, act)
    bounded("ft_act_bwd", out, R.act_bwd(yd, dyd, act), "n %d act %d%s" % (n, act, " pass 2" if n > THREADS_DEFAULT else ""))


@pytest.mark.parametrize("n", (ELT_N, PASS2_FLAT))
@pytest.mark.parametrize("op", (0, 1))
def test_eltwise(env, n, op):
    L = env
    a, b = R.normal((n,), 1), R.normal((n,), 2)
    assert R.eltwise_inputs_ok(a, b)
    ad, bd, out = cu(a), cu(b), nanbuf(n)
    call(L, "ft_eltwise", L.ptr(ad), L.ptr(bd), L.ptr(out), n, op)
    equal("ft_eltwise", out, R.eltwise(ad, bd, op)[0], "n %d op %d%s" % (n, op, " pass 2" if n > THREADS_DEFAULT else ""))


# ------------------------------------------------------------------------------------------------------------ beta-binomial prior, RAdam
def prior_lens(B, T, Lx, seed=0):
    il = torch.randint(1, Lx + 1, (B,), generator=R.gen(seed), dtype=torch.int32)
    ol = torch.randint(1, T + 1, (B,), generator=R.gen(seed + 1), dtype=torch.int32)
    il[-1], ol[-1] = Lx, T                                           # the last elements of the tensor are valid
    il[0], ol[0] = 1, 1
    return il, ol


@pytest.mark.parametrize("B,T,Lx", ((3, 17, 9), PASS2_PRIOR))
def test_beta_binomial_prior(env, B, T, Lx):
    L = env
    il, ol = prior_lens(B, T, Lx)
    ild, old = cu(il), cu(ol)
    out = nanbuf(B, T, Lx)
    call(L, "ft_beta_binomial_prior", L.ptr(ild), L.ptr(old), L.ptr(out), B, T, Lx, 0.05)
    ref, bound = R.beta_binomial_prior(ild, old, T, Lx, 0.05)
    bounded("ft_beta_binomial_prior", out, (ref, bound), "B %d T %d L %d%s" % (B, T, Lx, " pass 2" if B * T * Lx > THREADS_DEFAULT else ""))
    rows = ref.sum(-1)[ref.sum(-1) > 0]
    assert float((rows - 1).abs().max()) < 1e-9                      # the reference itself: every valid row is a distribution


@pytest.mark.parametrize("n", (RADAM_SMALL, PASS2_FLAT))
@pytest.mark.parametrize("rectified,clipped,wd", ((1, True, True), (0, False, False)))
def test_radam_single_step(env, n, rectified, clipped, wd):
    L = env
    p, g, m, v = radam_inputs(n)
    hp = dict(RADAM_HP, weight_decay=RADAM_HP["weight_decay"] if wd else 0.0, rectified=rectified)
    gsq = float((g.double() ** 2).sum().float()) * (1.0 if clipped else 1e-6)          # clip 1.0: norm above / below it
    pd, gd, md, vd = cu(p), cu(g), cu(m), cu(v)
    gn = torch.tensor([gsq], device="cuda")
    skipped = torch.zeros(1, dtype=torch.int32, device="cuda")
    ref = R.radam_step(pd, gd, md, vd, gnorm_sq=gsq, **hp)
    call(L, "ft_radam_step", L.ptr(pd), L.ptr(gd), L.ptr(md), L.ptr(vd), n, L.ptr(gn), hp["clip"], hp["lr"], hp["beta1"], hp["beta2"], hp["eps"],
         hp["weight_decay"], hp["step_size"], rectified, L.ptr(skipped))
    tag = "n %d rectified %d clipped %d wd %d%s" % (n, rectified, clipped, wd, " pass 2" if n > THREADS_RADAM else "")
    assert int(skipped) == 0
    for k, got in (("p", pd), ("m", md), ("v", vd)):
        bounded("ft_radam_step", got, ref[k], tag + " " + k)


def test_report_ratios():
    """the largest |err| / bound per entry point over the cases that ran (printed; the checks themselves are above)"""
    for k in sorted(RATIOS):
        print("%-26s %.4f" % (k, RATIOS[k]))
