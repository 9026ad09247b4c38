"""The judge of the inverse STFT's float64 test (tests/stft_ref64.py: istft_bound, ISTFT_MUTATIONS, istft64_ragged) held to its
purpose on the very inputs of test_gpu_istft_f64.py (tests/istft_cases.py), no GPU needed:

  * an honest fp32 inverse written with torch.fft (float32 irfft frames, float32 window product, overlap-add and envelope in
    ascending t in float32, the > FLT_MIN rule) lies inside the bound on every sample of every case -- hop 1 with 1 024
    overlapping frames and the samples beside a zero envelope, where the division amplifies, included.  Its largest ratio
    over the 25 dense cases is 0.0044 (n256_h64_w256_T66; 0.0007 at hop 1 / T 1100, 0.0025 beside the zero-envelope samples):
    the bound is a worst case, ~230 times what an honest computation needs, and was not fitted to it or to the kernels;
  * every wrong inverse leaves the bound on each case named for it in istft_cases.MUTATION_CASES, judged against that honest
    inverse (smallest: r8 keep_im_dc_nyquist at hop 1 / T 1100, 12.5 bounds; pow2 drop_first_halo at 1024 / 257, 12.8);
  * the ragged reference is the dense reference of each utterance's own frames, bit for bit, with zeros behind, and never
    reads the NaN behind a length;
  * the case list has the spans, seams, halo frames, staging rounds and zero-envelope samples its lines claim, computed
    from wss64 and a restatement of the index arithmetic that is itself checked against a brute-force cover."""
import numpy as np
import pytest
import torch

import istft_cases as cases
from stft_ref64 import (EPS32, ISTFT_MUTATIONS, TINY32, clamp_frames, default_span, hann64, inverse_bound, istft64, istft64_ragged,
                        istft_bound, istft_ratio, overlap_add_bound, wss64)


def honest32(M, P, n_fft, hop, w32):
    """[B, hop (T-1)] float32: the plain fp32 inverse.  Im of bins 0 and n_fft / 2 is dropped as irfft defines."""
    X = torch.polar(torch.from_numpy(M), torch.from_numpy(P))
    X[:, 0].imag.zero_()
    X[:, -1].imag.zero_()
    fr = (torch.fft.irfft(X, n=n_fft, dim=1) * torch.from_numpy(w32)[None, :, None]).numpy()
    assert fr.dtype == np.float32
    B, _, T = M.shape
    n = n_fft + hop * (T - 1)
    acc, wss, w2 = np.zeros((B, n), np.float32), np.zeros(n, np.float32), w32 * w32
    for t in range(T):
        acc[:, t * hop:t * hop + n_fft] += fr[:, :, t]
        wss[t * hop:t * hop + n_fft] += w2
    nz = wss > np.finfo(np.float32).tiny
    acc[:, nz] /= wss[nz]
    return acc[:, n_fft // 2:n - n_fft // 2]


@pytest.fixture(scope="module")
def dense():
    """id -> dict(M, P, w32, y64, zero, bound, honest): computed once, read by every test below."""
    out = {}
    for cid, c in zip(cases.IDS, cases.CASES):
        n_fft, hop, win, T, _ = c
        M, P = cases.spectrum(c)
        w32 = cases.window32(n_fft, win)
        y64, wss = istft64(M, P, n_fft, hop, win, w32)
        out[cid] = dict(M=M, P=P, w32=w32, y64=y64, zero=wss <= TINY32, bound=istft_bound(M, P, n_fft, hop, win, None, w32),
                        honest=honest32(M, P, n_fft, hop, w32))
    return out


@pytest.fixture(scope="module")
def ragged():
    out = {}
    for rid, c in zip(cases.RAGGED_IDS, cases.RAGGED_CASES):
        n_fft, hop, win, T, _ = c
        M, P, nf = cases.ragged_spectrum(c)
        w32 = cases.window32(n_fft, win)
        honest = np.zeros((len(nf), hop * (T - 1)), np.float32)
        for b, n in enumerate(nf):
            n = clamp_frames(n, T)
            if n >= 2:
                honest[b, :hop * (n - 1)] = honest32(M[b:b + 1, :, :n], P[b:b + 1, :, :n], n_fft, hop, w32)[0]
        out[rid] = dict(M=M, P=P, nf=nf, w32=w32, y64=istft64_ragged(M, P, n_fft, hop, win, nf, w32),
                        bound=istft_bound(M, P, n_fft, hop, win, nf, w32), honest=honest)
    return out


def test_inputs_are_what_the_list_says():
    for cid, c in zip(cases.IDS, cases.CASES):
        n_fft, hop, win, T, rng = c
        M, P = cases.spectrum(c)
        assert M.dtype == P.dtype == np.float32 and M.shape == P.shape == (3, n_fft // 2 + 1, T), cid
        assert 0 <= M[:, :, :T // 2].min() and M[:, :, :T // 2].max() < 2 and np.abs(P).max() <= rng, cid
        assert M[:, :, T // 2].mean() > 30 * M[:, :, T // 2 - 1].mean(), cid                # the loud frame
        assert (np.abs(P).max() > np.pi) == (rng > np.pi), cid
        assert 1 <= hop <= win <= n_fft and T >= 2 and cases.is_r8(n_fft, hop) == (cid in cases.R8_IDS), cid
    assert sum(c[4] > np.pi for c in cases.R8_CASES) == 1 and sum(c[4] > np.pi for c in cases.POW2_CASES) == 1
    assert len(cases.R8_CASES) == 13 and len(cases.POW2_CASES) == 12 and len(set(cases.IDS)) == 25


def test_honest_fp32_inverse_is_inside_the_bound(dense):
    worst = {}
    for cid, d in dense.items():
        r = istft_ratio(d["honest"], d["y64"], d["bound"])
        assert r.shape == d["y64"].shape and np.isfinite(d["bound"]).all(), cid
        beside = np.zeros_like(d["zero"])
        if d["zero"].any():                                                     # the neighbours of a zero-envelope sample
            i = np.nonzero(d["zero"])[0]
            beside[np.clip(np.concatenate([i - 1, i + 1]), 0, beside.size - 1)] = True
            beside &= ~d["zero"]
            assert np.all(d["honest"][:, d["zero"]] == 0) and np.all(d["y64"][:, d["zero"]] == 0), cid
        print("%-24s honest fp32 inverse: ratio %.4f%s" % (cid, r.max(), ", beside a zero envelope %.4f (%d samples)"
                                                           % (r[:, beside].max(), beside.sum()) if beside.any() else ""))
        assert r.max() <= 1.0, (cid, r.max())
        worst[cid] = float(r.max())
    top = max(worst, key=worst.get)
    print("honest fp32 inverse over %d cases: largest ratio %.4f (%s)" % (len(worst), worst[top], top))


def test_float64_reference_judges_itself_zero(dense, ragged):
    for d in list(dense.values()) + list(ragged.values()):
        assert istft_ratio(d["y64"], d["y64"], d["bound"]).max() == 0.0
    d = dense[cases.IDS[0]]
    bad = d["y64"].copy()
    bad[0, 0] = np.nan
    assert np.isinf(istft_ratio(bad, d["y64"], d["bound"])[0, 0])              # a sample left NaN fails
    z = dense[cases.ZERO_ENVELOPE_IDS[0]]
    assert (z["bound"][:, z["zero"]] == 0).all()                                # an exact zero of the window: nothing allowed
    off = z["y64"].copy()
    off[:, z["zero"]] = 1e-30
    assert np.isinf(istft_ratio(off, z["y64"], z["bound"])[:, z["zero"]]).all()


def test_overlap_add_term_is_the_derived_one(dense):
    """gamma_K S / wss + gamma_{K+1} |y| on a case small enough to write out: 1024 / 256 / T 3, K = 1 .. 3 frames a sample."""
    d = dense["n1024_h256_w1024_T3"]
    M, P, w = d["M"].astype(np.float64), d["P"].astype(np.float64), d["w32"].astype(np.float64)
    fr = np.fft.irfft(M * np.exp(1j * P), n=1024, axis=1) * w[None, :, None]
    u = 2.0 ** -24
    got = overlap_add_bound(d["M"], d["P"], 1024, 256, 1024, None, d["w32"])
    for n in (0, 100, 255, 256, 511):
        U = n + 512
        ts = [t for t in range(3) if 0 <= U - 256 * t < 1024 and w[U - 256 * t] != 0]
        S = sum(abs(fr[:, U - 256 * t, t]) for t in ts)
        wss = sum(w[U - 256 * t] ** 2 for t in ts)
        K = len(ts)
        gK, gK1 = K * u / (1 - K * u), (K + 1) * u / (1 - (K + 1) * u)
        want = (gK * S / wss + gK1 * np.abs(d["y64"][:, n])) / (1 - gK1)
        assert np.allclose(got[:, n], want, rtol=1e-12, atol=0), n
    assert len([t for t in range(3) if 512 - 256 * t >= 0]) == 3


def test_inverse_bound_at_1024_is_the_formula_griffin_lim_was_held_to():
    """test_gpu_griffin_lim.py's own inverse_bound, as it stood with its literals 10, 512 and 1024, gives the same numbers."""
    c = cases.BY_ID["n1024_h200_w200_T6"]
    M, _ = cases.spectrum(c)
    hop, win, T = 200, 200, 6
    Md = np.asarray(M, np.float64)
    A = (2 * Md.sum(axis=1) - Md[:, 0] - Md[:, 512]) / 1024
    w = hann64(win, 1024)
    env = np.zeros((3, 1024 + hop * (T - 1)))
    for t in range(T):
        env[:, t * hop:t * hop + 1024] += (np.abs(w)[None, :, None] * A[:, None, :])[:, :, t]
    wss = wss64(T, 1024, hop, win)
    nz = wss > TINY32
    env[:, nz] /= wss[nz]
    old = 8 * float(np.finfo(np.float32).eps) * 10 * env[:, 512:env.shape[1] - 512]
    assert np.array_equal(inverse_bound(M, 1024, hop, win), old)
    assert EPS32 == float(np.finfo(np.float32).eps)


def test_every_wrong_inverse_leaves_the_bound(dense, ragged):
    assert set(cases.MUTATION_CASES["r8"]) == set(cases.MUTATION_CASES["pow2"]) == set(ISTFT_MUTATIONS)
    for fam, ids in (("r8", cases.R8_IDS), ("pow2", cases.POW2_IDS)):
        for mut, named in cases.MUTATION_CASES[fam].items():
            assert named, (fam, mut)
            rs = []
            for cid in named:
                if cid in cases.RAGGED_IDS:
                    d, c = ragged[cid], cases.RAGGED_CASES[cases.RAGGED_IDS.index(cid)]
                    nf = d["nf"]
                else:
                    assert cid in ids, (fam, mut, cid)
                    d, c, nf = dense[cid], cases.BY_ID[cid], None
                n_fft, hop, win, T, _ = c
                wrong = ISTFT_MUTATIONS[mut](d["M"], d["P"], n_fft, hop, win, d["w32"], nf)
                assert wrong.shape == d["y64"].shape and not np.isnan(wrong).any(), (mut, cid)
                r = float(istft_ratio(d["honest"], wrong, d["bound"]).max())
                print("%-5s %-19s %-28s worst ratio %.3g" % (fam, mut, cid, r))
                assert r > 1.0, (fam, mut, cid, r)
                rs.append(r)
            print("%-5s %-19s closest %.3g" % (fam, mut, min(rs)))
    with pytest.raises(ValueError):
        d = dense[cases.IDS[0]]
        ISTFT_MUTATIONS["wss_batch_T"](d["M"], d["P"], 1024, 256, 1024, d["w32"])


def test_ragged_reference_is_the_dense_reference_of_the_slice(ragged):
    for rid, c in zip(cases.RAGGED_IDS, cases.RAGGED_CASES):
        n_fft, hop, win, T, _ = c
        d = ragged[rid]
        assert d["nf"] == [T, 2, 1, 0, T + 5, 17]
        assert not np.isnan(d["y64"]).any() and not np.isnan(d["bound"]).any()
        for b, n in enumerate(d["nf"]):
            n = clamp_frames(n, T)
            assert n == min(max(d["nf"][b], 1), T)
            assert np.isnan(d["M"][b, :, n:]).all() and np.isnan(d["P"][b, :, n:]).all()
            assert not np.isnan(d["M"][b, :, :n]).any()
            end = hop * (n - 1)
            assert np.all(d["y64"][b, end:] == 0) and np.all(d["bound"][b, end:] == 0)
            if n >= 2:
                m, p = d["M"][b:b + 1, :, :n], d["P"][b:b + 1, :, :n]
                assert np.array_equal(d["y64"][b, :end], istft64(m, p, n_fft, hop, win, d["w32"])[0][0])
                assert np.array_equal(d["bound"][b, :end], istft_bound(m, p, n_fft, hop, win, None, d["w32"])[0])
            else:
                assert end == 0
        r = istft_ratio(d["honest"], d["y64"], d["bound"])
        print("%s honest fp32 inverse, utterance by utterance: ratio %.4f" % (rid, r.max()))
        assert r.max() <= 1.0


def _covering(n_fft, hop, T, u0, u1):
    """Brute force: the frames with a tap on some sample of [u0, u1)."""
    s = np.arange(T) * hop
    return np.nonzero((s <= u1 - 1) & (s + n_fft - 1 >= u0))[0]


def test_case_list_has_the_geometry_it_claims():
    assert set(cases.EXPECT) == set(cases.IDS)
    for cid, c in zip(cases.IDS, cases.CASES):
        n_fft, hop, win, T, _ = c
        g = cases.geometry(n_fft, hop, T)
        for s in g:                                                             # the restated index arithmetic against a plain cover
            assert not s["behind"] and s["zero_fill"] == 0, cid                 # a dense launch has neither
            cov = _covering(n_fft, hop, T, s["u0"], s["u1"])
            assert cov[0] == s["t_lo"] and cov[-1] == s["t_hi"] and len(cov) == s["t_hi"] - s["t_lo"] + 1, (cid, s)
        got = dict(spans=len(g), zeros=int(cases.zero_envelope(n_fft, hop, win, T).sum()), t_lo=max(s["t_lo"] for s in g),
                   halo=max(s["halo"] for s in g), rounds=max(s["rounds"] for s in g), partial=any(s["partial"] for s in g))
        assert got == cases.EXPECT[cid], (cid, got)
    E = cases.EXPECT
    # the seams: the output ends exactly on one, and one hop past it
    assert 256 * 16 == default_span(1024, 256) and E["n1024_h256_w1024_T17"]["spans"] == 1
    assert 256 * 17 == default_span(1024, 256) + 256 and E["n1024_h256_w1024_T18"] == dict(spans=2, zeros=0, t_lo=15, halo=3,
                                                                                           rounds=3, partial=True)
    assert 64 * 64 == default_span(256, 64) == 4096 and E["n256_h64_w256_T65"]["spans"] == 1
    assert 64 * 65 == 4096 + 64 and E["n256_h64_w256_T66"]["spans"] == 2
    assert 300 * 14 == 4096 + 104 and E["n2048_h300_w1200_T15"]["spans"] == 2
    assert 4096 * 2 == 2 * 4096 and E["n4096_h4096_w4096_T3"]["spans"] == 2     # ends on its second seam
    # hop 13: 21 spans, up to 79 halo frames; hop 1: a 1 023-frame halo, and t_lo > 0 only beyond 1 024 frames
    assert (E["n1024_h13_w1024_T331"]["spans"], E["n1024_h13_w1024_T331"]["halo"]) == (21, 79)
    assert E["n1024_h1_w1024_T1100"]["halo"] == 1023 and E["n1024_h1_w1024_T1100"]["t_lo"] > 0 == E["n1024_h1_w1024_T40"]["t_lo"]
    assert E["n256_h1_w201_T4300"]["halo"] == 255 and E["n256_h1_w201_T4300"]["t_lo"] > 0
    assert 1 * (2 - 1) == 1                                                     # n1024_h1_w1024_T2: one output sample
    # a span shorter than the workgroup's 256 threads: the u < u1 guards carry the result
    assert [i for i in cases.R8_IDS if default_span(1024, cases.BY_ID[i][1]) < 256] == [
        "n1024_h13_w1024_T331", "n1024_h7_w800_T2", "n1024_h1_w1024_T2", "n1024_h1_w1024_T40", "n1024_h1_w1024_T1100"]
    # zero-envelope samples: the three r8 cases of the list, three pow2 ones; beside them the envelope is 2e-8 .. 4e-7
    assert [E[i]["zeros"] for i in ("n1024_h256_w256_T5", "n1024_h200_w200_T6", "n1024_h128_w128_T9")] == [4, 5, 8]
    assert cases.ZERO_ENVELOPE_IDS == ["n1024_h256_w256_T5", "n1024_h200_w200_T6", "n1024_h128_w128_T9", "n512_h512_w512_T9",
                                       "n1024_h512_w512_T12", "n4096_h4096_w4096_T3"]
    for cid in cases.ZERO_ENVELOPE_IDS[:3]:
        n_fft, hop, win, T, _ = cases.BY_ID[cid]
        wss = wss64(T, n_fft, hop, win, cases.window32(n_fft, win))[512:-512]
        i = np.nonzero(wss <= TINY32)[0]
        assert np.all(wss[i] == 0)
        near = wss[np.concatenate([i - 1, i + 1])]
        assert 2e-8 <= near.min() and near.max() <= 4e-7, (cid, near.min(), near.max())
    # every branch of the table in test_gpu_istft_f64.py has a dense case (the ragged ones: below)
    assert any(E[i]["t_lo"] > 0 for i in cases.R8_IDS) and any(E[i]["t_lo"] > 0 for i in cases.POW2_IDS)
    assert any(not E[i]["partial"] for i in cases.R8_IDS) and any(E[i]["partial"] for i in cases.R8_IDS)


def test_ragged_batches_reach_the_ragged_branches():
    for c in cases.RAGGED_CASES:
        n_fft, hop, win, T, _ = c
        counts = cases.ragged_counts(T)
        assert min(counts) < 1 and max(counts) > T and 1 in counts and 2 in counts and T in counts     # both sides of the clamp
        per = [cases.geometry(n_fft, hop, clamp_frames(n, T), T) for n in counts]
        assert all(len(g) == 2 for g in per)
        assert all(s["behind"] for g in (per[2], per[3]) for s in g)            # one frame: nothing but zeros to write
        assert any(s["behind"] for s in per[5]) and not per[5][0]["behind"]     # a span wholly behind a live utterance
        assert per[1][0]["zero_fill"] > 0                                       # the u >= u1 zero fill inside a live span
        assert not any(s["behind"] or s["zero_fill"] for g in (per[0], per[4]) for s in g)
    r8, p2 = cases.RAGGED_CASES
    assert cases.geometry(*r8[:2], 17, 18)[0]["zero_fill"] == 0                 # 1024 / 256: 17 frames end on the seam
    assert cases.geometry(*p2[:2], 17, 48)[0]["zero_fill"] == 2048              # 512 / 128: they end inside the first span
