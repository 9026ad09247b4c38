"""Style transfer on the device (flowtron_amd/style.py, csrc/style.hip; the reference's inference_style_transfer.ipynb):
the posterior kernels against the float64 restatement (tests/style_ref64.py) and against the notebook's own output
(tests/golden/style_posterior.pt), the invariances the accumulator promises, sampling, Flowtron.latents, and the whole chain
reference utterance -> posterior -> sample -> infer with no tolerance."""
import os

import numpy as np
import pytest
import torch

import style_ref64 as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AGGREGATIONS = ("batch", "time_and_batch")
LAYOUTS = ("bmt", "tbm")


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(GOLDEN, "style_posterior.pt"), weights_only=False)


def padded(zs, T, layout="bmt"):
    """The utterances as one device batch z [B, 80, T] with NaN behind every length (a frame that is read shows in the result):
    contiguous ('bmt'), or the permuted view of a time-major [T, B, 80] tensor ('tbm': what the forward's z looks like)."""
    z = torch.full((len(zs), zs[0].shape[0], T), float("nan"))
    for b, u in enumerate(zs):
        z[b, :, :u.shape[1]] = u
    if layout == "bmt":
        return z.cuda()
    zt = z.permute(2, 0, 1).contiguous().cuda()
    v = zt.permute(1, 2, 0)
    assert v.stride(1) == 1 and not v.is_contiguous()
    return v


def lengths(zs):
    return [u.shape[1] for u in zs]


def posterior(zs, agg, n_frames, lambd, T=None, layout="bmt"):
    from flowtron_amd.style import StylePosterior
    p = StylePosterior(aggregation=agg, n_frames=n_frames if agg == "batch" else None, lambd=lambd)
    p.add(padded(zs, T or max(lengths(zs)), layout), lengths(zs))
    assert p.count == len(zs)
    return p


def assert_within(out, ref, S, what):
    out = out.cpu().numpy().astype(np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert np.isfinite(out).all(), "%s: a frame behind an utterance's end was read" % (what,)
    err, bound = np.abs(out - ref), R.kernel_bound(ref, S)
    print(what, "max err %.3e" % err.max(), "max err / bound %.3f" % (err / bound).max())
    assert (err <= bound).all(), (what, float((err / bound).max()))


@pytest.mark.parametrize("lambd", [1e-4, 1.0])
@pytest.mark.parametrize("n_frames", [1, 20, 100])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("agg", AGGREGATIONS)
def test_kernels_against_float64(golden, agg, layout, n_frames, lambd):
    """mean():  |out - ref64| <= 2^-24 |ref64| + 2^-45 S  (one rounding to fp32 + slack for the float64 accumulation), S the
    same expression over |z|; sample(eps, sigma = 0.7, n = 3): the same with |sigma eps| added into S.  n_frames = 1 and 20 cut
    the longer utterances, 100 wraps every one of them."""
    zs = golden["random"]["z"]
    assert lengths(zs) == [37, 1, 20, 36, 7]
    p = posterior(zs, agg, n_frames, lambd, layout=layout)
    ref, S = R.posterior_mean([u.numpy() for u in zs], lambd, agg, n_frames)
    mu = p.mean()
    assert mu.dtype == torch.float32 and mu.is_cuda
    assert_within(mu, ref, S, "mean %s %s n_frames %d lambd %g" % (agg, layout, n_frames, lambd))
    eps = torch.randn(3, 80, n_frames, generator=torch.Generator().manual_seed(n_frames))
    out = p.sample(n=3, sigma=0.7, eps=eps.cuda(), n_frames=n_frames if agg == "time_and_batch" else None)
    ref_s, S_s = R.sample(ref, S, eps.numpy(), 0.7)
    assert_within(out, ref_s, S_s, "sample %s %s n_frames %d lambd %g" % (agg, layout, n_frames, lambd))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_exact_case_equals_the_notebook_bit_for_bit(golden, layout):
    g = golden["exact"]
    assert len(g["mu"]) == 6
    for k, want in g["mu"].items():
        agg, nf = k.split("/")
        got = posterior(g["z"], agg, int(nf), g["lambd"], layout=layout).mean()
        assert got.shape == want.shape and torch.equal(got.cpu(), want), k


@pytest.mark.parametrize("agg", AGGREGATIONS)
def test_split_and_padding_invariance(golden, agg):
    """the same reference set in one call, in 2 + 3, in five calls of one utterance and padded to T = 64 instead of 37: the same
    bits (every accumulator element has one owner, a time sum's order depends on the utterance's length alone)"""
    from flowtron_amd.style import StylePosterior
    zs = golden["random"]["z"]
    lens = lengths(zs)
    want = posterior(zs, agg, 100, 1e-4).mean()
    z = padded(zs, 37)
    for cuts in ([0, 2, 5], [0, 1, 2, 3, 4, 5]):
        p = StylePosterior(aggregation=agg, n_frames=100 if agg == "batch" else None)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            p.add(z[lo:hi], lens[lo:hi])
        assert p.count == 5 and torch.equal(p.mean(), want), cuts
    assert torch.equal(posterior(zs, agg, 100, 1e-4, T=64).mean(), want)
    assert torch.equal(posterior(zs, agg, 100, 1e-4, T=64, layout="tbm").mean(), posterior(zs, agg, 100, 1e-4, layout="tbm").mean())


def test_sampling(golden):
    zs = golden["random"]["z"]
    p = posterior(zs, "batch", 20, 1e-4)
    mu = p.mean()
    out = p.sample(n=4, sigma=0.0)
    assert out.shape == (4, 80, 20) and out.dtype == torch.float32
    for s in range(4):
        assert torch.equal(out[s], mu)

    def draw(seed):
        return p.sample(n=2, sigma=1.0, generator=torch.Generator(device="cuda").manual_seed(seed))
    a, b, c = draw(5), draw(5), draw(6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert bool(torch.isfinite(a).all()) and float((a - mu).std()) > 0.5          # unit-variance draws around the mean
    with pytest.raises(ValueError, match="n_frames"):
        p.sample(n_frames=20)
    with pytest.raises(ValueError, match="eps"):
        p.sample(n=2, eps=torch.zeros(1, 80, 20).cuda())

    q = posterior(zs, "time_and_batch", None, 1e-4)
    mq = q.mean()
    assert mq.shape == (80, 1)
    with pytest.raises(ValueError, match="n_frames"):
        q.sample()
    eps = torch.randn(2, 80, 7, generator=torch.Generator().manual_seed(3))
    flat = q.sample(n=2, sigma=0.0, eps=eps.cuda(), n_frames=7)
    assert flat.shape == (2, 80, 7) and torch.equal(flat, mq[None].expand(2, 80, 7))          # the one mu[m] in every column
    out = q.sample(n=2, sigma=0.5, eps=eps.cuda(), n_frames=7)
    ref, S = R.posterior_mean([u.numpy() for u in zs], 1e-4, "time_and_batch")
    ref_s, S_s = R.sample(ref, S, eps.numpy(), 0.5)
    assert_within(out, ref_s, S_s, "time_and_batch sample")


# ---- the model side: Flowtron.latents and the chain into infer ------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import flowtron
    from oracle import synth
    os.environ["FLOWTRON_MFMA"] = "f32"
    cfg = dict(synth.SMALL_MODEL_CONFIG, n_flows=2)
    m = flowtron.Flowtron(**cfg)
    m.load_state_dict(synth.make_state_dict(cfg, seed=41))           # coupling weights NOT zero: z != mel
    return m.cuda().eval(), cfg


def batch_one(m, b, i):
    """the batch-1 forward of utterance i, as the notebook runs it -> z [1, M, len]"""
    il, ol = int(b["in_lens"][i]), int(b["out_lens"][i])
    with torch.no_grad():
        z = m(b["mel"][i:i + 1, :, :ol], b["speaker_ids"][i:i + 1], b["text"][i:i + 1, :il], torch.tensor([il]).cuda(),
              torch.tensor([ol]).cuda())[0]
    return z.permute(1, 2, 0)


def test_latents_equal_the_batch_one_forwards(model):
    """three utterances, text lengths NOT descending: each utterance's z within 5e-5 of its own batch-1 forward (the bound
    test_full_config_invertibility_and_padding_invariance puts on the forward's independence of what an utterance is batched
    with), zeros behind its length, the caller's order kept"""
    from oracle import synth
    m, cfg = model
    out_lens, in_lens = [40, 23, 9], [7, 12, 5]
    b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synth.make_batch(cfg, out_lens, in_lens, seed=41, with_prior=False).items()}
    z = m.latents(b["mel"], b["speaker_ids"], b["text"], in_lens, b["out_lens"])
    assert z.shape == (3, 80, 40) and z.dtype == torch.float32 and not z.requires_grad
    for i, n in enumerate(out_lens):
        z1 = batch_one(m, b, i)
        d = (z[i, :, :n] - z1[0]).abs().max().item()
        print("utterance %d: |z - batch-1 z| max %.3e, |z - mel| max %.3e" % (i, d, (z1[0] - b["mel"][i, :, :n]).abs().max().item()))
        assert d < 5e-5, (i, d)
        assert (z1[0] - b["mel"][i, :, :n]).abs().max().item() > 1e-2           # the flows do something
        assert float(z[i, :, n:].abs().sum()) == 0.0
    m.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            m.latents(b["mel"], b["speaker_ids"], b["text"], in_lens, b["out_lens"])
    finally:
        m.eval()
    with pytest.raises(ValueError, match="out_lens"):
        m.latents(b["mel"], b["speaker_ids"], b["text"], in_lens, [41, 23, 9])


def test_end_to_end_without_tolerance(model):
    """one reference utterance, ratio = 1 (c = 0.5 exactly), 'batch' aggregation at its own length, sigma = 0: the sampled z IS
    0.5 * the batch-1 forward's z, bit for bit, and infer turns both into the same mel; again with the utterance added twice and
    lambd = 2 (ratio 1, the mean of two equal values exact)"""
    from flowtron_amd.style import StylePosterior
    from oracle import synth
    m, cfg = model
    n, lt = 23, 9
    b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synth.make_batch(cfg, [n], [lt], seed=43, with_prior=False).items()}
    want = 0.5 * batch_one(m, b, 0)
    sid = torch.zeros(1, dtype=torch.long).cuda()
    text = b["text"][:, :lt]
    mel_want, _ = m.infer(want, sid, text, gate_threshold=1.0)
    assert mel_want.shape == (1, 80, n) and bool(torch.isfinite(mel_want).all())
    for times, lambd in ((1, 1.0), (2, 2.0)):
        p = StylePosterior(aggregation="batch", n_frames=n, lambd=lambd)
        for _ in range(times):
            z = p.add_utterances(m, b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
        assert p.count == times and z.shape == (1, 80, n)
        got = p.sample(sigma=0.0)
        assert got.shape == (1, 80, n) and torch.equal(got, want), (times, (got - want).abs().max().item())
        mel, _ = m.infer(got, sid, text, gate_threshold=1.0)
        assert torch.equal(mel, mel_want)
    # force_speaker_id: the notebook's sid * 0 + force_speaker_id
    p = StylePosterior(aggregation="batch", n_frames=n, lambd=1.0)
    z_forced = p.add_utterances(m, b["mel"], b["speaker_ids"] * 0 + 2, b["text"], b["in_lens"], b["out_lens"], force_speaker_id=1)
    assert torch.equal(z_forced, m.latents(b["mel"], b["speaker_ids"] * 0 + 1, b["text"], b["in_lens"], b["out_lens"]))
