"""Style-transfer posterior without a GPU: the float64 restatement (tests/style_ref64.py) against the reference notebook's own
output (tests/golden/style_posterior.pt, tests/golden/make_golden_style.py), and the argument errors StylePosterior raises on
the host before anything reaches the device."""
import os

import numpy as np
import pytest
import torch

import style_ref64 as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(GOLDEN, "style_posterior.pt"), weights_only=False)


def _key(k):
    agg, nf = k.split("/")
    return agg, int(nf)


def test_restatement_equals_the_notebook_bit_for_bit_on_the_exact_case(golden):
    """entries k / 16, lengths powers of two, K = 4, c = 0.5: every fp32 operation of the notebook is exact, so float64 must
    give the same numbers"""
    g = golden["exact"]
    zs = [z.numpy() for z in g["z"]]
    assert [z.shape[1] for z in zs] == [8, 16, 32, 4]
    assert sorted(g["mu"]) == sorted("%s/%d" % (a, n) for a in ("batch", "time_and_batch") for n in (1, 20, 50))
    for k, mu in g["mu"].items():
        agg, nf = _key(k)
        ref, _ = R.posterior_mean(zs, g["lambd"], agg, nf)
        assert mu.dtype == torch.float32 and tuple(mu.shape) == ref.shape, k
        assert np.array_equal(mu.numpy().astype(np.float64), ref), k


def test_restatement_within_the_notebooks_fp32_error_on_the_random_case(golden):
    """(K + 5) 2^-24 S for 'batch', (T_max + K + 5) 2^-24 S for 'time_and_batch' (style_ref64.notebook_bound): derived from the
    notebook's operations, not measured"""
    g = golden["random"]
    zs = [z.numpy() for z in g["z"]]
    assert [z.shape[1] for z in zs] == [37, 1, 20, 36, 7]
    assert sorted(g["mu"]) == ["batch/100", "time_and_batch/100"]
    for k, mu in g["mu"].items():
        agg, nf = _key(k)
        ref, S = R.posterior_mean(zs, g["lambd"], agg, nf)
        assert tuple(mu.shape) == ref.shape, k
        err = np.abs(mu.numpy().astype(np.float64) - ref)
        bound = R.notebook_bound(S, len(zs), agg, 37)
        print(k, "max err %.3e" % err.max(), "max err / bound %.3f" % (err / bound).max())
        assert (err <= bound).all(), (k, float((err / bound).max()))


def test_host_side_argument_errors():
    from flowtron_amd.style import StylePosterior
    with pytest.raises(ValueError, match="n_frames"):
        StylePosterior(aggregation="batch")
    with pytest.raises(ValueError, match="aggregation"):
        StylePosterior(aggregation="time", n_frames=4)
    with pytest.raises(ValueError, match="lambd"):
        StylePosterior(n_frames=4, lambd=0.0)
    StylePosterior(aggregation="time_and_batch")                       # n_frames is not needed there
    p = StylePosterior(n_frames=10)
    z = torch.zeros(2, 80, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # a CPU tensor is refused, not emulated
        p.add(z, [6, 3])
    with pytest.raises(ValueError, match="mel channels"):
        p.add(torch.zeros(2, 79, 6), [6, 3])
    with pytest.raises(ValueError, match="B, M, T"):
        p.add(torch.zeros(80, 6), [6])
    with pytest.raises(ValueError, match="lengths"):
        p.add(z, [6, 0])
    with pytest.raises(ValueError, match="lengths"):
        p.add(z, [7, 3])
    with pytest.raises(ValueError, match="lengths"):
        p.add(z, torch.tensor([6, 3, 1]))
    with pytest.raises(ValueError, match="lengths"):
        p.add(z, None)
    assert p.count == 0
    with pytest.raises(ValueError, match="no reference utterance"):
        p.mean()
    with pytest.raises(ValueError, match="no reference utterance"):
        p.sample()


def test_c_abi_refuses_bad_arguments_before_the_device():
    """FT_EINVAL from the entry points themselves, with host memory standing in for the buffers: nothing may be launched"""
    import ctypes as C
    from flowtron_amd import _lib as L
    lib = L.lib()
    z = (C.c_float * 64)()
    lens = (C.c_int32 * 2)()
    acc = (C.c_double * 9)()
    out = (C.c_float * 64)()
    pz, pl, pa, po = (C.addressof(x) for x in (z, lens, acc, out))
    ok = dict(z=pz, sb=32, sm=4, st=1, lens=pl, acc=pa, B=2, M=8, T=4, nf=4, mode=L.STYLE_BATCH)

    def accumulate(**kw):
        a = dict(ok, **kw)
        return lib.ft_style_accumulate(a["z"], a["sb"], a["sm"], a["st"], a["lens"], a["acc"], a["B"], a["M"], a["T"], a["nf"],
                                       a["mode"], None)
    for kw in (dict(z=None), dict(lens=None), dict(acc=None), dict(B=0), dict(M=0), dict(T=0), dict(nf=0), dict(mode=2),
               dict(st=-1), dict(acc=pa + 4)):
        assert accumulate(**kw) == -1, kw
        assert b"ft_style_accumulate" in lib.ft_last_error()

    oks = dict(acc=pa, eps=po, out=po, S=1, M=8, nf=4, K=2, lambd=1.0, sigma=1.0, mode=L.STYLE_BATCH)

    def sample(**kw):
        a = dict(oks, **kw)
        return lib.ft_style_sample(a["acc"], a["eps"], a["out"], a["S"], a["M"], a["nf"], a["K"], a["lambd"], a["sigma"], a["mode"],
                                   None)
    for kw in (dict(acc=None), dict(out=None), dict(S=0), dict(M=0), dict(nf=0), dict(K=0), dict(lambd=0.0), dict(lambd=-1.0),
               dict(lambd=float("nan")), dict(mode=-1), dict(eps=None, S=2), dict(acc=pa + 4)):
        assert sample(**kw) == -1, kw
        assert b"ft_style_sample" in lib.ft_last_error()
