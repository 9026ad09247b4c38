"""Gaussian-mixture prior without a GPU: the float64 restatement (tests/gm_ref64.py) against the REAL reference's results in
tests/golden/gm_small.pt, the sharpness of its bound, the model's state_dict layout, and the argument checks of the new entry points
(all made on the host, before any device call).

Tolerance of the restatement against the golden loss: the reference evaluates the loss in fp32 -- about ten roundings per element
(exp, sqrt, log, the products) and a torch.sum whose vectorised pairwise tree is under 2 log2(N) deep for the N < 2^13 terms here.
REF_ROUNDINGS = 40 whole ulps of the mean |term| covers both; the gradients that are compared are sums of B rows of per-utterance
sums over up to T M terms, each with the same element error: the same 40 ulps of sum |terms|."""
import ctypes
import os
import pickle

import pytest
import torch

import gm_fixture as GF
import gm_ref64 as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_ROUNDINGS = 40


@pytest.fixture(scope="module")
def gm():
    return torch.load(os.path.join(GOLDEN, "gm_small.pt"), weights_only=False)


def _inputs(name, case):
    o = case["out"]
    lens = torch.tensor(GF.CASES[name]["out_lens"])
    return o["z"], o["mean"], o["log_var"], o["prob"], lens, o["log_s"]


@pytest.mark.parametrize("name", list(GF.CASES))
def test_restatement_reproduces_reference_loss(gm, name):
    z, mean, log_var, prob, lens, log_s = _inputs(name, gm[name])
    loss, _ = R.mixture_nll_fwd(z, mean, log_var, prob, lens, log_s)
    # the log-domain form equals the reference's linear-domain formula in float64 ...
    lin = R.reference_formula_nll(z, mean, log_var, prob, lens, log_s)
    assert abs(float(loss - lin)) < 1e-12 * abs(float(lin))
    # ... and the reference's own fp32 result within its rounding
    m = R.frame_mask(lens, z.shape[0])[:, :, None]
    l = R._chain(torch.where(m, z, torch.zeros(())), mean, log_var, prob)["l"]
    mean_term = float(((l.abs() + sum(x.double().abs() for x in log_s)) * m).sum()) / float(m.sum() * z.shape[2])
    assert abs(float(loss) - gm[name]["nll"].item()) < REF_ROUNDINGS * R.U * mean_term, (float(loss), gm[name]["nll"].item())


@pytest.mark.parametrize("name", list(GF.CASES))
def test_restatement_reproduces_reference_gradients(gm, name):
    """The bias gradients of the mixture's heads are column sums of the likelihood's gradients: prob_layer.bias = sum_b softmax'
    (dprob), mean_layer.bias = sum_b dmean, log_var_layer.bias = sum_b dlog_var (the loss enters the total with weight 1)."""
    case = gm[name]
    z, mean, log_var, prob, lens, log_s = _inputs(name, case)
    g = R.mixture_nll_bwd(z, mean, log_var, prob, lens, 1.0)

    def check(key, ref64, mag):
        ref = case["grads"][key]["full"].double()
        tol = REF_ROUNDINGS * R.U * mag + 1e-9
        assert bool(((ref64 - ref).abs() <= tol).all()), (key, float(((ref64 - ref).abs() / tol).max()))

    dlogits, _ = R.softmax_rows_bwd(prob, g["dprob"][0])
    mag = (prob.double() * g["dprob"][0].abs()).sum(0) + (prob.double() * (prob.double() * g["dprob"][0].abs()).sum(1, keepdim=True)).sum(0)
    check("gaussian_mixture.prob_layer.linear_layer.bias", dlogits.sum(0), mag)
    if not case["cfg"]["fixed_gaussian"]:
        M = z.shape[2]
        k = R._chain(torch.where(R.frame_mask(lens, z.shape[0])[:, :, None], z, torch.zeros(())), mean, log_var, prob)
        # magnitudes of the summed terms: |dmean| terms are r |d| / var, |dlog_var| terms r |1/2 + a d^2|, both / (n M)
        nm = float(lens.sum()) * M
        q = torch.exp(k["u"] - k["l"][..., None]) * k["P"] * R.frame_mask(lens, z.shape[0])[:, :, None, None]
        check("gaussian_mixture.mean_layer.linear_layer.bias", g["dmean"][0].sum(0).reshape(-1),
              ((q * k["d"].abs() * k["inv"]).sum((0, 1)) / nm).reshape(-1))
        check("gaussian_mixture.log_var_layer.linear_layer.bias", g["dlog_var"][0].sum(0).reshape(-1),
              ((q * (0.5 + k["a"] * k["d2"]).abs()).sum((0, 1)) / nm).reshape(-1))


def test_bound_is_sharp(gm):
    """a reference that is wrong by the smallest amount that matters lands outside the kernel's bound: one component's log_var off
    by one bf16 ulp, or one frame past each length counted"""
    for name in ("fixed", "learned"):
        z, mean, log_var, prob, lens, log_s = _inputs(name, gm[name])
        z = z.clone()
        z[R.frame_mask(lens, z.shape[0]).logical_not()] = 0.3            # (defined values behind the lengths for the extra-frame reference)
        loss, bound = R.mixture_nll_fwd(z, mean, log_var, prob, lens, log_s)
        assert float(bound) < 1e-4 * abs(float(loss))
        lv = log_var.clone()
        c = int(prob.sum(0).argmax())                                   # the component that carries the most weight
        lv[:, :, c] += torch.where(lv[:, :, c] != 0, lv[:, :, c].abs() * 2.0 ** -8, torch.full_like(lv[:, :, c], 2.0 ** -8))
        wrong, _ = R.mixture_nll_fwd(z, mean, lv, prob, lens, log_s)
        assert abs(float(wrong - loss)) > R.SHARP * float(bound), (name, float(wrong - loss), float(bound))
        wrong, _ = R.mixture_nll_fwd(z, mean, log_var, prob, lens, log_s, extra_frame=True)
        assert abs(float(wrong - loss)) > R.SHARP * float(bound), (name, float(wrong - loss), float(bound))
        gb = R.mixture_nll_bwd(z, mean, log_var, prob, lens, 1.0)
        gw = R.mixture_nll_bwd(z, mean, lv, prob, lens, 1.0)
        for key in ("dz", "dmean", "dlog_var", "dprob"):
            assert R.ratio(gw[key][0], gb[key][0], gb[key][1]) > R.SHARP, (name, key)


def test_pool_softmax_sample_restatements():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, 3, 5, generator=g)
    lens = torch.tensor([4, 7, 1])
    y, _ = R.time_pool_fwd(x, lens)
    xz = x.double() * R.frame_mask(lens, 7)[:, :, None]
    assert torch.allclose(y, xz.mean(0))                               # flowtron.py:437-439 on the zero-padded output (T == max length)
    y9, _ = R.time_pool_fwd(torch.cat([x, torch.full((2, 3, 5), float("nan"))]), lens)
    assert torch.equal(y9, y)                                          # extra padding: still divided by the longest length, never read
    dy = torch.randn(3, 5, generator=g)
    xg = x.double().requires_grad_(True)
    ((xg * R.frame_mask(lens, 7)[:, :, None]).mean(0) * dy.double()).sum().backward()
    assert torch.allclose(R.time_pool_bwd(dy, lens, 7)[0], xg.grad)
    lg = torch.randn(4, 3, generator=g).double().requires_grad_(True)
    sm = torch.softmax(lg, 1)
    assert torch.allclose(R.softmax_rows_fwd(lg.detach().float())[0], torch.softmax(lg.detach().float().double(), 1))
    w = torch.randn(4, 3, generator=g).double()
    (sm * w).sum().backward()
    assert torch.allclose(R.softmax_rows_bwd(sm.detach(), w)[0], lg.grad)
    mean, lv = torch.randn(2, 5, 3, generator=g), torch.randn(2, 5, 3, generator=g)
    rows, comp = torch.tensor([1, 0]), torch.tensor([2, 0])
    eps = torch.randn(2, 5, 4, generator=g)
    out, _ = R.mixture_sample(mean, lv, rows, comp, eps, 0.7)
    assert torch.allclose(out[1, 3], mean[0, 3, 0].double() + 0.7 * torch.exp(0.5 * lv[0, 3, 0].double()) * eps[1, 3].double())
    assert torch.equal(R.mixture_sample(mean, lv, rows, comp, None, 0.0)[0][0, :, 0], mean[1, :, 2].double())


@pytest.mark.parametrize("name", list(GF.CASES))
def test_state_dict_layout_and_round_trips(gm, name):
    import flowtron
    case = gm[name]
    m = flowtron.Flowtron(**case["cfg"])
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in case["spec"]]
    # the mel encoder's 16 entries, then the prob head's 2 and either the 2 buffers or the 4 entries of the learned heads
    assert len(sd) == 68 + (20 if case["cfg"]["fixed_gaussian"] else 22)
    m.load_state_dict(GF.state_dict_of(name, case), strict=True)
    for k in case["buffers"]:
        assert torch.equal(m.state_dict()[k], case["buffers"][k])
    m2 = pickle.loads(pickle.dumps(m))                                 # train.py pickles the whole module into its checkpoints
    assert type(m2.mel_encoder).__module__ == "flowtron" and list(m2.state_dict()) == list(sd)
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), m.state_dict().values()))


def test_fixed_gaussians_as_the_reference_generates_them():
    import flowtron
    gmix = flowtron.GaussianMixture(64, 4, 80, True, 3.0)
    mean = gmix.mean
    assert tuple(mean.shape) == (1, 80, 4) and tuple(gmix.log_var.shape) == (1, 80, 4) and not bool(gmix.log_var.any())
    assert bool(((mean == 0) | (mean == 3.0)).all()) and mean.sum(1).tolist() == [[3.0] * 4]       # one channel per component
    assert len(set(mean[0].argmax(0).tolist())) == 4                                             # drawn without replacement
    assert gmix.generate_prob().tolist() == [[1.0]]
    assert [n for n, _ in gmix.named_parameters()] == ["prob_layer.linear_layer.weight", "prob_layer.linear_layer.bias"]


def test_without_components_nothing_changes():
    import flowtron
    from oracle import synth
    for n in (0, 1):
        m = flowtron.Flowtron(**dict(synth.SMALL_MODEL_CONFIG, n_components=n))
        assert len(m.state_dict()) == 68 and not hasattr(m, "mel_encoder") and not hasattr(m, "gaussian_mixture")
    crit = flowtron.FlowtronLoss(1.0, True, True, False, 0.0, -8)      # a config with n_components 1 sets gm_loss and builds no mixture
    with pytest.raises(ValueError, match="n_components"):
        crit((torch.zeros(2, 1, 80), [], None, [], [], None, None, None), None, torch.tensor([1]), torch.tensor([2]))


def test_entry_points_refuse_bad_arguments_on_the_host():
    """FT_EINVAL before any device call: this machine has no GPU, so a device call would fail with another code (or crash)"""
    from flowtron_amd import _lib as L
    lib = L.lib()
    P = ctypes.c_void_p(64)                                            # any non-NULL address: never dereferenced
    T, B, M = 4, 3, 80

    def fwd(C=4, Bm=1, z=P, M=M):
        return lib.ft_mixture_nll_fwd(z, P, P, P, None, 0, M, P, P, P, P, T, B, M, C, Bm, None)

    def bwd(C=4, Bm=1, z=P, work=P):
        return lib.ft_mixture_nll_bwd(z, P, P, P, P, P, P, P, P, P, P, P, work, T, B, M, C, Bm, None)

    def sample(C=4, mean=P, rows=P):
        return lib.ft_mixture_sample(mean, P, rows, P, P, P, 2, M, 5, C, 3, 1.0, None)

    EINVAL = -1
    for f in (fwd, bwd):
        assert f(C=1) == EINVAL and f(C=65) == EINVAL and f(z=None) == EINVAL and f(Bm=2) == EINVAL and f(Bm=0) == EINVAL
        assert b"invalid argument" in lib.ft_last_error()
    assert fwd(M=257) == EINVAL and bwd(work=None) == EINVAL
    assert fwd(C=64, M=96) == EINVAL                                   # the constants of 96 x 64 do not fit a workgroup's LDS
    assert sample(C=1) == EINVAL and sample(C=65) == EINVAL and sample(mean=None) == EINVAL and sample(rows=None) == EINVAL
    for f in (lib.ft_softmax_rows_fwd, ):
        assert f(P, P, 3, 1, None) == EINVAL and f(P, P, 3, 65, None) == EINVAL and f(None, P, 3, 4, None) == EINVAL
    assert lib.ft_softmax_rows_bwd(P, P, P, 3, 1, None) == EINVAL and lib.ft_softmax_rows_bwd(P, None, P, 3, 4, None) == EINVAL
    assert lib.ft_softmax_rows_bwd(P, P, P, 3, 65, None) == EINVAL
    assert lib.ft_time_pool_fwd(None, P, P, 4, 3, 8, None) == EINVAL and lib.ft_time_pool_fwd(P, P, P, 0, 3, 8, None) == EINVAL
    assert lib.ft_time_pool_bwd(None, P, P, 4, 3, 8, None) == EINVAL and lib.ft_time_pool_bwd(P, P, P, 4, 0, 8, None) == EINVAL
    assert lib.ft_mixture_nll_work_floats(862, 32, 80, 8) == 36 * 32 * (2 * 80 * 8 + 8)
    assert lib.ft_abi_version() == 15                                  # functions were added; no signature or struct changed


def test_cpu_tensors_are_refused():
    import flowtron
    from flowtron_amd import mixture, ops
    z, mean, prob, lens = torch.zeros(2, 1, 80), torch.zeros(1, 80, 2), torch.full((1, 2), 0.5), torch.tensor([2], dtype=torch.int32)
    for call in (lambda: ops.MixtureNLLFn.apply(z, mean, mean, prob, lens),
                 lambda: ops.TimePoolFn.apply(z, lens),
                 lambda: ops.SoftmaxRowsFn.apply(prob),
                 lambda: ops.mixture_sample(mean, mean, torch.zeros(1, dtype=torch.int32), 3, 0.0),
                 lambda: mixture.sample_component(mean, mean, 1, 3),
                 lambda: flowtron.MelEncoder(64)(torch.zeros(1, 80, 4), torch.tensor([4]))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="no mixture"):
        from oracle import synth
        mixture.mixture_parameters(flowtron.Flowtron(**synth.SMALL_MODEL_CONFIG), z, [1])
