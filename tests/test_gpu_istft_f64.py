"""Both inverse STFT kernels on the MI355X -- istft_r8_k (csrc/stft_r8.hip: n_fft 1024, hop <= 256) and istft_pow2_k<LH>
(csrc/stft_pow2.hip: every other power-of-two setting) -- against the float64 inverse of tests/stft_ref64.py on the very float32
window the kernels read, sample by sample: |y - y64| <= istft_bound (FFT term + the derived overlap-add term; held to an honest
fp32 inverse, and to every wrong inverse, by test_istft_ref64_cpu.py without a GPU).  No sample is left out; the dense launches
go through STFT.inverse and once more straight into a buffer of NaN, the ragged ones straight to ft_istft_*_ragged with counts
the host wrapper would refuse.  Inputs: tests/istft_cases.py.

Which case enters which branch (csrc/stft_r8.hip, csrc/stft_pow2.hip; computed from the geometry by test_istft_ref64_cpu.py):

  branch                                              r8 cases (1024 / hop / win / T)              pow2 cases (n_fft / hop / win / T)
  the output ends on a span seam                      256/1024/17                                  256/64/256/65, 512/512/512/9,
                                                                                                   4096/1024/4096/5, 4096/4096/4096/3
  ... one hop past it (a span of one hop)             256/1024/18                                  256/64/256/66
  ... inside a later span                             13/1024/331, 1/1024/40, 1/1024/1100          256/1/201/4300, 512/160/401/40,
                                                                                                   1024/257/1024/20, 1024/512/512/12,
                                                                                                   2048/300/1200/15, 4096/333/3001/14
  halo frames of a later span with t_lo = 0           1/1024/40 (40), 13/1024/331 (72),            -
                                                      1/1024/1100 (1 008)
  halo frames with t_lo > 0                           256/1024/18 (3), 13/1024/331 (79),           256/64/256/66 (3), 256/1/201/4300 (255),
                                                      1/1024/1100 (1 023, t_lo up to 577)          512/160/401/40, 1024/257/1024/20, ...
  a full last staging round                           1/1024/40 (every span: 40 = 5 x 8),          one span each of 256/1/201/4300,
                                                      3 spans of 13/.., 32 of 1/1024/1100          512/160/401/40, 1024/512/512/12, 2048/300/..
  a partial last staging round                        every other case                             every case
  many staging rounds                                 1/1024/1100 (130), 13/1024/331 (12)          256/1/201/4300 (1 056)
  span shorter than the 256 threads (u < u1 guards)   13/.., 7/800/2, 1/../2 (one sample), 1/../40, 1/../1100    -
  T = 2, T = 3                                        256/1024/2, 256/1024/3, 255/1024/3, 7/800/2, 1/1024/2      4096/1024/4096/2, 4096/4096/4096/3
  wss > FLT_MIN false (stored undivided)              256/256/5 (4), 200/200/6 (5), 128/128/9 (8)  512/512/512/9 (8), 1024/512/512/12 (11),
                                                                                                   4096/4096/4096/3 (2)
  wss > FLT_MIN true                                  every case                                   every case
  phases in [-60, 60] (sincosf's range reduction)     255/1024/3                                   512/160/401/40
  ragged: the clamp min(max(n, 1), T)                 counts 0 and T + 5 of ragged 1024/256/18     the same of ragged 512/128/48
  ragged: early return, span wholly behind            n = 17 (ends on the seam), n = 1, 2          n = 17, 2, 1 (second span), n = 1 (both)
  ragged: the u >= u1 zero fill in a live span        n = 2 (3 840 samples)                        n = 2 (3 968), n = 17 (2 048)
  ragged: n = 1, nothing but zeros                    counts 1 and 0                               counts 1 and 0

Measured on an MI355X, 2026-10-21 (pytest -s prints every figure; profiles/istft_f64_pytest_gpu.log holds them all):

  largest |gpu - f64| / bound   r8 0.0033 (255/1024/3; 0.0007 at hop 1 / T 1100, <= 0.0012 beside a zero envelope)
                                pow2 0.0047 (256/64/256/65; 0.0026 at 256/1/201/4300, <= 0.0020 beside a zero envelope)
                                ragged 0.0018 (r8), 0.0035 (pow2), exact zeros behind every utterance
  closest wrong inverse         r8 keep_im_dc_nyquist, 12.5 bounds (hop 1 / T 1100); then symmetric_hann 17.9 (hop 13)
                                pow2 drop_first_halo, 12.8 bounds (1024/257/1024/20); then keep_im_dc_nyquist 51.3 (n_fft 4096)
The honest fp32 inverse of test_istft_ref64_cpu.py reaches 0.0044 of the same bound: the kernels round like it.  No defect was
found in either kernel."""
import functools

import numpy as np
import pytest
import torch

import audio_processing
import istft_cases as cases
from flowtron_amd import _lib as L
from stft_ref64 import ISTFT_MUTATIONS, TINY32, clamp_frames, istft64, istft64_ragged, istft_bound, istft_ratio

pytestmark = pytest.mark.gpu


def launch(st, m, ph, nf=None):
    """ft_istft_{r8,pow2}{,_ragged} straight through the library into a buffer of NaN: y [B, hop (T-1)]."""
    B, _, T = m.shape
    y = torch.full((B, st.hop_length * (T - 1)), float("nan"), device=m.device, dtype=torch.float32)
    head = (L.ptr(m), L.ptr(ph)) + ((L.ptr(nf),) if nf is not None else ()) + (L.ptr(st.fft_window), L.ptr(y), B, T)
    if st.fast_path():
        name, geo = "ft_istft_r8", (st.hop_length,)
    else:
        name, geo = "ft_istft_pow2", (st.filter_length, st.hop_length, st.win_length)
    name += "_ragged" if nf is not None else ""
    L.check(getattr(L.lib(), name)(*head, *geo, L.stream()), name)
    return y


def module_for(case):
    n_fft, hop, win, _, _ = case
    st = audio_processing.STFT(n_fft, hop, win).cuda()
    assert st.fast_path() == cases.is_r8(n_fft, hop) and (st.fast_path() or st.pow2_path())
    assert np.array_equal(st.fft_window.cpu().numpy(), cases.window32(n_fft, win))
    return st


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(M, P, w32, y64, zero-envelope mask, bound) of a dense case: computed once, never written to."""
    c = cases.BY_ID[cid]
    n_fft, hop, win, T, _ = c
    M, P = cases.spectrum(c)
    w32 = cases.window32(n_fft, win)
    y64, wss = istft64(M, P, n_fft, hop, win, w32)
    return M, P, w32, y64, wss <= TINY32, istft_bound(M, P, n_fft, hop, win, None, w32)


@functools.lru_cache(maxsize=None)
def device_output(cid):
    """The kernel's output for a dense case [B, hop (T-1)] float64, through STFT.inverse; the second launch, straight into
    NaN, must give the same bits and leave no NaN."""
    c = cases.BY_ID[cid]
    M, P = reference(cid)[:2]
    st = module_for(c)
    m, ph = torch.from_numpy(M).cuda(), torch.from_numpy(P).cuda()
    y = st.inverse(m, ph)
    assert y.shape == (M.shape[0], 1, c[1] * (c[3] - 1)), (cid, y.shape)
    again = launch(st, m, ph)
    assert not torch.isnan(again).any(), (cid, int(torch.isnan(again).sum()))
    assert torch.equal(y[:, 0], again), cid
    return y[:, 0].cpu().double().numpy()


@functools.lru_cache(maxsize=None)
def ragged_run(rid):
    c = cases.RAGGED_CASES[cases.RAGGED_IDS.index(rid)]
    n_fft, hop, win, T, _ = c
    M, P, nf = cases.ragged_spectrum(c)
    st = module_for(c)
    m, ph = torch.from_numpy(M).cuda(), torch.from_numpy(P).cuda()
    nfd = torch.tensor(nf, dtype=torch.int32).cuda()
    y = launch(st, m, ph, nfd)
    assert torch.equal(y, launch(st, m, ph, nfd)) or torch.isnan(y).any(), rid          # NaN: reported by the test itself
    w32 = cases.window32(n_fft, win)
    return dict(c=c, M=M, P=P, nf=nf, st=st, m=m, ph=ph, y=y, w32=w32, y64=istft64_ragged(M, P, n_fft, hop, win, nf, w32),
                bound=istft_bound(M, P, n_fft, hop, win, nf, w32))


@pytest.mark.parametrize("cid", cases.IDS)
def test_dense_every_sample(cid):
    M, P, w32, y64, zero, bound = reference(cid)
    got = device_output(cid)
    ratio = istft_ratio(got, y64, bound)
    print("%-24s max |gpu - f64| / bound = %.4f, %d samples, %d with wss <= FLT_MIN" % (cid, ratio.max(), ratio.size, zero.sum()))
    assert ratio.shape == y64.shape and ratio.max() <= 1.0, (cid, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))
    assert int(zero.sum()) == cases.EXPECT[cid]["zeros"], cid
    if cid in cases.ZERO_ENVELOPE_IDS:
        # stored undivided: the reference's undivided value, which for this window's exact zero tap is 0, and nothing is allowed
        assert zero.any() and np.all(bound[:, zero] == 0) and np.all(y64[:, zero] == 0)
        assert np.all(got[:, zero] == 0), cid
        i = np.nonzero(zero)[0]
        beside = np.unique(np.clip(np.concatenate([i - 1, i + 1]), 0, zero.size - 1))
        print("%-24s beside the zero envelope: ratio %.4f" % (cid, ratio[:, beside].max()))


@pytest.mark.parametrize("rid", cases.RAGGED_IDS)
def test_ragged_every_utterance(rid):
    r = ragged_run(rid)
    n_fft, hop, win, T, _ = r["c"]
    y = r["y"]
    assert not torch.isnan(y).any(), (rid, int(torch.isnan(y).sum()))
    got = y.cpu().double().numpy()
    for b, n in enumerate(r["nf"]):
        n = clamp_frames(n, T)
        end = hop * (n - 1)
        assert np.all(got[b, end:] == 0), (rid, b)                              # exact zeros from hop (n - 1) to the end
        if n >= 2:
            dense = r["st"].inverse(r["m"][b:b + 1, :, :n].contiguous(), r["ph"][b:b + 1, :, :n].contiguous())
            assert torch.equal(y[b, :end], dense[0, 0]), (rid, b)               # bit for bit the dense call on its own frames
        else:
            assert end == 0 and np.all(got[b] == 0)
    ratio = istft_ratio(got, r["y64"], r["bound"])
    print("%-28s max |gpu - f64| / bound per utterance: %s" % (rid, " ".join("%.4f" % v for v in ratio.max(axis=1))))
    assert ratio.max() <= 1.0, (rid, ratio.max(axis=1))


@pytest.mark.parametrize("fam", ["r8", "pow2"])
def test_device_output_is_outside_every_wrong_inverse(fam):
    """Sharpness on the kernel's own output: with a wrong inverse as the reference, some sample of every case named for it
    leaves the bound."""
    assert set(cases.MUTATION_CASES[fam]) == set(ISTFT_MUTATIONS)
    closest = {}
    for mut, named in cases.MUTATION_CASES[fam].items():
        rs = []
        for cid in named:
            if cid in cases.RAGGED_IDS:
                r = ragged_run(cid)
                n_fft, hop, win, T, _ = r["c"]
                got, bound = r["y"].cpu().double().numpy(), r["bound"]
                wrong = ISTFT_MUTATIONS[mut](r["M"], r["P"], n_fft, hop, win, r["w32"], r["nf"])
            else:
                n_fft, hop, win, T, _ = cases.BY_ID[cid]
                M, P, w32, _, _, bound = reference(cid)
                got = device_output(cid)
                wrong = ISTFT_MUTATIONS[mut](M, P, n_fft, hop, win, w32)
            ratio = float(istft_ratio(got, wrong, bound).max())
            print("%-5s %-19s %-28s |gpu - wrong| / bound = %.3g" % (fam, mut, cid, ratio))
            assert ratio > 1.0, (fam, mut, cid, ratio)
            rs.append(ratio)
        closest[mut] = min(rs)
        print("%-5s %-19s closest %.3g" % (fam, mut, closest[mut]))
    mut = min(closest, key=closest.get)
    print("%s: the closest wrong inverse is %s at %.3g bounds" % (fam, mut, closest[mut]))
