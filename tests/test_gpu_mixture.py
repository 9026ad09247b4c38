"""Gaussian-mixture prior on the device (-m gpu): the kernels of csrc/mixture.hip element by element against float64 within the
bounds tests/gm_ref64.py derives from their fp32 operation chain, their determinism, and the model (mel encoder, mixture heads,
gm_loss) against the REAL reference's results in tests/golden/gm_small.pt.  fp32 operand mode unless stated.

Kernel shapes: C in {2, 3, 8, 64} (64 = the limit, 3 no power of two), mean / log_var rows 1 and B, B in {1, 3, 33}, T in {1, 7, 130}
(24 frames per workgroup at M 80: one chunk, a part of one, six), M 80; lengths include 1 and T in unsorted order; NaN behind every
length in z and every log_s.  Model tolerances are DESIGN section 2's for goldens in fp32 mode: outputs 1e-4 max-abs, NLL 1e-5
relative, gradients 1e-4 relative L2 (analytically zero ones absolutely), and 2e-2 relative NLL in bf16 mode."""
import ctypes as C
import os

import pytest
import torch

import gm_fixture as GF
import gm_ref64 as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M = 80
NAN = float("nan")
ZERO_GRAD_SLACK = 1e-5

# name -> (C, rows of mean / log_var are B?, B, T, lengths | None = seeded, kind)
KERNEL_CASES = {
    "c2_b1_t1": (2, False, 1, 1, [1], "plain"),
    "c3_b3_t7_rows": (3, True, 3, 7, [7, 1, 4], "plain"),
    "c8_b33_t130": (8, False, 33, 130, None, "plain"),
    "c64_b3_t130_rows": (64, True, 3, 130, [57, 130, 1], "plain"),
    "c64_b33_t7": (64, False, 33, 7, None, "plain"),
    "c3_b33_t130_rows_far": (3, True, 33, 130, None, "far"),
    "c8_b3_t7_no_param_grads": (8, True, 3, 7, [4, 7, 1], "null"),
}
_CACHE = {}


def _case(name):
    """inputs on the device, the kernels' outputs and the float64 references, computed once per case"""
    if name in _CACHE:
        return _CACHE[name]
    from flowtron_amd import _lib as L
    Cn, rows_b, B, T, lens, kind = KERNEL_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if lens is None:
        lens = torch.randint(1, T + 1, (B,), generator=g).tolist()
        lens[3], lens[17], lens[30] = T, 1, T                          # the extremes, not in order
    Bm = B if rows_b else 1
    dev = "cuda"
    z = torch.randn(T, B, M, generator=g) * 1.5 - 2.0
    mean = torch.randn(Bm, M, Cn, generator=g) * 2.0 - 2.0
    log_var = torch.randn(Bm, M, Cn, generator=g) * 0.7
    if kind == "far":
        # every z lies about 40 sigma from two of the three components: their responsibilities underflow to exactly 0 and only the
        # shift by the largest exponent keeps the sum finite
        z = torch.randn(T, B, M, generator=g) * 0.5
        mean = torch.stack([torch.zeros(Bm, M), torch.full((Bm, M), 40.0), torch.full((Bm, M), -45.0)], 2)
        log_var = torch.zeros(Bm, M, Cn)
    prob = torch.softmax(torch.randn(B, Cn, generator=g) * 1.5, 1)
    out = torch.randn(2, T, B, 2 * M, generator=g) * 0.3               # log_s: strided views of the coupling outputs
    pad = R.frame_mask(torch.tensor(lens), T).logical_not()
    z[pad] = NAN
    out[:, pad] = NAN
    z, mean, log_var, prob, out = (t.to(dev) for t in (z, mean, log_var, prob, out))
    log_s = [out[0][..., :M], out[1][..., :M]]
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    gscale = torch.tensor([0.7], device=dev)
    lib = L.lib()
    f32 = dict(device=dev, dtype=torch.float32)
    acc, loss = torch.empty(8, **f32), torch.empty((), **f32)
    work = torch.empty(lib.ft_mixture_nll_work_floats(T, B, M, Cn), **f32)
    ls_ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in log_s])

    def fwd():
        L.check(lib.ft_mixture_nll_fwd(z.data_ptr(), mean.data_ptr(), log_var.data_ptr(), prob.data_ptr(), ls_ptrs, 2, 2 * M,
                                       lens_d.data_ptr(), acc.data_ptr(), work.data_ptr(), loss.data_ptr(), T, B, M, Cn, Bm,
                                       L.stream()), "ft_mixture_nll_fwd")

    def bwd():
        o = {"dz": torch.full((T, B, M), NAN, **f32), "dls": torch.full((T, B, M), NAN, **f32)}
        if kind != "null":
            o.update(dmean=torch.full((B, M, Cn), NAN, **f32), dlog_var=torch.full((B, M, Cn), NAN, **f32),
                     dprob=torch.full((B, Cn), NAN, **f32))
        p = {k: v.data_ptr() for k, v in o.items()}
        L.check(lib.ft_mixture_nll_bwd(z.data_ptr(), mean.data_ptr(), log_var.data_ptr(), prob.data_ptr(), lens_d.data_ptr(),
                                       acc.data_ptr(), gscale.data_ptr(), p["dz"], p["dls"], p.get("dmean"), p.get("dlog_var"),
                                       p.get("dprob"), work.data_ptr(), T, B, M, Cn, Bm, L.stream()), "ft_mixture_nll_bwd")
        return o

    fwd()
    got = bwd()
    got["loss"] = loss.clone()
    lens_l = lens_d.long()
    ref = R.mixture_nll_bwd(z, mean, log_var, prob, lens_l, 0.7)
    ref["loss"] = R.mixture_nll_fwd(z, mean, log_var, prob, lens_l, log_s)
    torch.cuda.synchronize()
    _CACHE[name] = dict(got=got, ref=ref, bwd=bwd, z=z, mean=mean, log_var=log_var, prob=prob, lens=lens)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_mixture_nll_kernels_vs_float64(name):
    c = _case(name)
    worst = {}
    for key, val in c["got"].items():
        ref, bound = c["ref"][key]
        assert tuple(val.shape) == tuple(ref.shape), key
        worst[key] = R.ratio(val, ref, bound)
    print("mixture_nll %s: worst error / bound %s" % (name, {k: "%.3f" % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst
    if KERNEL_CASES[name][5] == "far":
        # the case does what it is for: the far components' exponents lie below expf's range in fp32, the result is finite
        z, mean = c["z"], c["mean"]
        assert float(((torch.nan_to_num(z)[..., None] - mean[None]) ** 2 / 2)[..., 1:].min()) > 104.0
        assert bool(torch.isfinite(c["got"]["loss"]))
    if KERNEL_CASES[name][5] == "null":
        assert set(c["got"]) == {"dz", "dls", "loss"}


def test_mixture_nll_backward_is_deterministic():
    for name in ("c8_b33_t130", "c3_b33_t130_rows_far"):
        c = _case(name)
        again = c["bwd"]()
        for key, val in again.items():
            a, b = val, c["got"][key]
            assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and not bool(torch.isnan(a).any()), (name, key)
        assert len(again) == 5


@pytest.mark.parametrize("T,B,W,lens", [(9, 3, 70, [4, 7, 1]), (1, 1, 64, [1]), (130, 33, 64, None)])
def test_time_pool_vs_float64(T, B, W, lens):
    """the divisor is the batch's longest length, also with padding appended behind it (T 9, longest 7); NaN behind every length"""
    from flowtron_amd import ops
    g = torch.Generator().manual_seed(T * 100 + W)
    if lens is None:
        lens = torch.randint(1, T + 1, (B,), generator=g).tolist()
        lens[5], lens[20] = T, 1
    x = torch.randn(T, B, W, generator=g)
    x[R.frame_mask(torch.tensor(lens), T).logical_not()] = NAN
    x = x.cuda().requires_grad_(True)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    y = ops.TimePoolFn.apply(x, lens_d)
    ref, bound = R.time_pool_fwd(x.detach(), lens_d.long())
    r_f = R.ratio(y.detach(), ref, bound)
    dy = torch.randn(B, W, generator=g).cuda()
    y.backward(dy)
    ref_b, bound_b = R.time_pool_bwd(dy, lens_d.long(), T)
    r_b = R.ratio(x.grad, ref_b, bound_b)
    print("time_pool T %d B %d W %d: worst error / bound fwd %.3f bwd %.3f" % (T, B, W, r_f, r_b))
    assert r_f <= 1.0 and r_b <= 1.0
    if T == 9:
        assert torch.allclose(y.double(), torch.nan_to_num(x.detach().double()).sum(0) / 7.0, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("Cn", [2, 3, 8, 64])
@pytest.mark.parametrize("B", [1, 33])
def test_softmax_rows_vs_float64(B, Cn):
    from flowtron_amd import ops
    g = torch.Generator().manual_seed(B * 100 + Cn)
    x = (torch.randn(B, Cn, generator=g) * 3.0).cuda().requires_grad_(True)
    y = ops.SoftmaxRowsFn.apply(x)
    ref, bound = R.softmax_rows_fwd(x.detach())
    dy = torch.randn(B, Cn, generator=g).cuda()
    y.backward(dy)
    ref_b, bound_b = R.softmax_rows_bwd(y.detach(), dy)
    r_f, r_b = R.ratio(y.detach(), ref, bound), R.ratio(x.grad, ref_b, bound_b)
    print("softmax_rows B %d C %d: worst error / bound fwd %.3f bwd %.3f" % (B, Cn, r_f, r_b))
    assert r_f <= 1.0 and r_b <= 1.0


# ------------------------------------------------------------------------------------------------------------ model
@pytest.fixture(scope="module")
def gm():
    return torch.load(os.path.join(GOLDEN, "gm_small.pt"), weights_only=False)


def _model(name, case, mode="f32"):
    import flowtron
    os.environ["FLOWTRON_MFMA"] = mode
    m = flowtron.Flowtron(**case["cfg"])
    m.load_state_dict(GF.state_dict_of(name, case), strict=True)
    m = m.cuda().train()
    keep = [k.float().permute(2, 0, 1).contiguous().cuda() for k in case["keep_masks"]]      # [B,C,L] -> [L,B,C]
    m.encoder.dropout_masks, m.mel_encoder.dropout_masks = keep[:3], keep[3:]
    b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in GF.batch_of(name).items()}
    return m, b


def mad(a, b):
    return (a.detach().float().cpu() - b.detach().float().cpu()).abs().max().item()


def _step(m, b):
    import flowtron
    out = m(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"], b["attn_prior"])
    crit = flowtron.FlowtronLoss(1.0, True, True, True, 0.01, -8)
    nll, gl, ctc = crit(out, b["gate_target"], b["in_lens"], b["out_lens"])
    (nll + gl + 0.01 * ctc).sum().backward()
    return out, nll, gl, ctc


@pytest.mark.parametrize("name", list(GF.CASES))
def test_model_vs_reference_golden(gm, name):
    case = gm[name]
    m, b = _model(name, case)
    mel_before = b["mel"].clone()
    out, nll, gl, ctc = _step(m, b)
    assert torch.equal(b["mel"], mel_before)                           # the reference zero-fills its input in place; this one only reads
    o = case["out"]
    assert mad(out[0], o["z"]) < 1e-4 and mad(out[2], o["gate"]) < 1e-4
    for i in range(2):
        assert mad(out[1][i], o["log_s"][i]) < 1e-4 and mad(out[3][i], o["attn"][i]) < 1e-5 and mad(out[4][i], o["logprob"][i]) < 5e-4
    for j, key in ((5, "mean"), (6, "log_var"), (7, "prob")):
        assert tuple(out[j].shape) == tuple(o[key].shape), key
        assert mad(out[j], o[key]) < 1e-4, (key, mad(out[j], o[key]))
    assert abs(nll.item() - case["nll"].item()) < 1e-5 * abs(case["nll"].item()), (nll.item(), case["nll"].item())
    assert abs(gl.item() - case["gate_loss"].item()) < 1e-5
    assert abs(ctc.item() - case["ctc"].item()) < 1e-4 * max(1.0, abs(case["ctc"].item()))
    worst = ("", 0.0)
    assert [k for k, _ in m.named_parameters()] == list(case["grads"])
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        ref, view, norm = GF.grad_view(case["grads"][k], p.grad.cpu())
        if "convolutions" in k and k.endswith("conv.bias"):
            # analytically zero (the instance norm behind the convolution removes the bias): rounding residue on both sides,
            # compared absolutely with the slack tests/test_gpu_model.py gives the same tensors
            assert (view - ref).norm().item() <= ZERO_GRAD_SLACK and ref.norm().item() <= ZERO_GRAD_SLACK, k
            continue
        denom = max(ref.norm().item(), 1e-5 * ref.numel() ** 0.5)
        r = (view - ref).norm().item() / denom
        if norm is not None:
            r = max(r, abs(p.grad.double().norm().item() - norm) / max(norm, 1e-5 * p.numel() ** 0.5))
        if r > worst[1]:
            worst = (k, r)
    print("gm golden %s: nll %.7f (reference %.7f), worst gradient %s %.2e" % (name, nll.item(), case["nll"].item(), worst[0], worst[1]))
    assert worst[1] < 1e-4, worst


def test_model_bf16_mode(gm):
    case = gm["learned"]
    try:
        m, b = _model("learned", case, "bf16")
        out, nll, gl, ctc = _step(m, b)
    finally:
        os.environ["FLOWTRON_MFMA"] = "f32"
    assert bool(torch.isfinite(nll)) and abs(nll.item() - case["nll"].item()) < 2e-2 * abs(case["nll"].item()), nll.item()
    new = [(k, p) for k, p in m.named_parameters() if k.startswith(("mel_encoder.", "gaussian_mixture."))]
    assert len(new) == 22                                              # 16 of the mel encoder, 6 of the three learned heads
    for k, p in new:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert float(p.grad.abs().max()) > 0 or k.endswith("conv.bias"), k


def test_one_optimizer_step(gm):
    from radam import RAdam
    case = gm["learned"]
    m, b = _model("learned", case)
    opt = RAdam(m.parameters(), lr=1e-3)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    _step(m, b)
    opt.step()
    torch.cuda.synchronize()
    arena = opt.arena.flat_grad
    lo, hi = arena.data_ptr(), arena.data_ptr() + arena.numel() * 4
    for k, p in m.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        if k.startswith(("mel_encoder.", "gaussian_mixture.")):
            assert lo <= p.grad.data_ptr() < hi, k                     # the flat arena holds the new parameters' gradients
            if not k.endswith("conv.bias"):                            # (analytically zero gradient: the instance norm removes the bias)
                assert not torch.equal(p.detach(), before[k]), k


# ------------------------------------------------------------------------------------------------------------ sampler
def test_sampler_vs_float64_and_infer(gm):
    from flowtron_amd import mixture, ops
    g = torch.Generator().manual_seed(5)
    mean, log_var = (torch.randn(3, M, 5, generator=g) * 2.0).cuda(), torch.randn(3, M, 5, generator=g).cuda()
    rows = torch.tensor([2, 0, 1, 1], dtype=torch.int32, device="cuda")
    comp = torch.tensor([4, 0, 3, 3], dtype=torch.int32, device="cuda")
    eps = torch.randn(4, M, 37, generator=g).cuda()
    out = ops.mixture_sample(mean, log_var, comp, 37, 0.8, rows, eps)
    ref, bound = R.mixture_sample(mean, log_var, rows, comp, eps, 0.8)
    r = R.ratio(out, ref, bound)
    print("mixture_sample: worst error / bound %.3f" % r)
    assert tuple(out.shape) == (4, M, 37) and r <= 1.0
    mu = mixture.sample_component(mean, log_var, [4, 0, 3, 3], 37, sigma=0.0, rows=[2, 0, 1, 1])
    assert torch.equal(mu, mean[rows.long(), :, comp.long()][:, :, None].expand(-1, -1, 37))
    gen = torch.Generator(device="cuda").manual_seed(1)
    a = mixture.sample_component(mean[:1], log_var[:1], 2, 11, sigma=0.5, generator=gen)
    gen.manual_seed(1)
    assert torch.equal(a, mixture.sample_component(mean[:1], log_var[:1], 2, 11, sigma=0.5, generator=gen)) and tuple(a.shape) == (1, M, 11)
    with pytest.raises(ValueError, match="component"):
        mixture.sample_component(mean, log_var, 5, 3, rows=0)
    with pytest.raises(ValueError, match="rows"):
        mixture.sample_component(mean, log_var, 1, 3, rows=3)
    # the model's own mixture, utterances in any order, and a sample through infer
    case = gm["fixed"]
    m, b = _model("fixed", case)
    m.eval()
    m.encoder.dropout_masks = m.mel_encoder.dropout_masks = None       # (the hook outranks eval(): the masks are this batch's)
    mean_m, lv_m, prob_m = mixture.mixture_parameters(m, b["mel"], b["out_lens"])
    assert tuple(mean_m.shape) == (1, M, 4) and tuple(prob_m.shape) == (3, 4) and torch.allclose(prob_m.sum(1), torch.ones(3, device="cuda"))
    perm = torch.tensor([2, 0, 1], device="cuda")
    _, _, prob_p = mixture.mixture_parameters(m, b["mel"][perm], b["out_lens"][perm])
    assert mad(prob_p, prob_m[perm]) < 1e-5
    zs = mixture.sample_component(mean_m, lv_m, 1, 6, sigma=0.5)
    mel, attn = m.infer(zs, b["speaker_ids"][:1], b["text"][:1, :4], gate_threshold=1.0)
    assert tuple(mel.shape) == (1, M, 6) and bool(torch.isfinite(mel).all())
    lat = m.latents(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"], b["attn_prior"])
    assert tuple(lat.shape) == tuple(b["mel"].shape)                   # latents() keeps its result (and skips the mel encoder)
