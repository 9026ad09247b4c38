"""Sample-rate conversion on the device (ft_resample_ragged, csrc/resample.hip): every output sample against the float64
restatement of the definition (tests/resample_ref64.py) inside a bound built from that sample's own sum |h x|, the ragged
form against each utterance resampled alone bit for bit, DC gain and impulse response, launch counts, and the data path
end to end: a mixed-rate filelist through Data(resample=True), DataCollate and the mel slot's `.cuda()`, then one training
step of a small model on that batch."""
import ctypes

import numpy as np
import pytest
import torch

import audio_processing
import resample_case as C
import resample_ref64 as R
from call_count import count_calls
from flowtron_amd import _lib as L
from flowtron_amd import audio as A
from flowtron_amd.data import Data, DataCollate

pytestmark = pytest.mark.gpu

PAIRS = [(24000, 22050), (16000, 22050), (44100, 22050), (48000, 8000), (8000, 48000), (44100, 48000)]
EPS = 2.0 ** -24


def check_against_float64(x, orig, new):
    """x [B, N] fp32 on the host: resample on the device and hold EVERY output sample to
    |y - y64| <= (K + 3) 2^-24 sum_k |h_k x_k|: the taps' rounding to fp32 (1), one rounding per tap of the fmaf chain (K) and
    2 of slack; y64 and the sum come from the float64 definition with unrounded taps."""
    K = A.resample_taps(orig, new)[4]
    y = audio_processing.resample(torch.from_numpy(x).cuda(), orig, new).cpu().numpy().astype(np.float64)
    assert y.shape == (x.shape[0], R.out_len(x.shape[1], orig, new))
    worst = 0.0
    for b in range(x.shape[0]):
        y64, mag = R.resample64(x[b], orig, new)
        bound = (K + 3) * EPS * mag
        err = np.abs(y[b] - y64)
        assert (err <= bound).all(), (orig, new, x.shape, b, int(np.argmax(err - bound)), float((err - bound).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


# ---- 6. dense against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", PAIRS)
def test_dense_matches_float64(orig, new):
    rs = np.random.RandomState(orig % 1000 + new % 1000)
    x = rs.standard_normal((3, 4001)).astype(np.float32)
    print("%d -> %d: worst error / bound %.3f" % (orig, new, check_against_float64(x, orig, new)))


@pytest.mark.parametrize("orig,new", PAIRS)
def test_dense_matches_float64_at_the_edges(orig, new):
    # the filter hangs over both ends of the signal at once (N < K), and N straddles one output tile / one input span
    K = A.resample_taps(orig, new)[4]
    rs = np.random.RandomState(7)
    for N in (1, 2, K - 1, 160, 161):
        check_against_float64(rs.standard_normal((3, N)).astype(np.float32), orig, new)


def test_more_outputs_than_one_tile_and_workgroups_than_the_grid():
    # 1 200 rows of 1 100 samples: > 1024 (row, tile) pairs, so workgroups walk several tiles; every row equals the row alone
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.standard_normal((1200, 1100)).astype(np.float32)).cuda()
    y = audio_processing.resample(x, 16000, 22050)
    for b in (0, 1, 599, 1023, 1024, 1199):
        assert torch.equal(y[b], audio_processing.resample(x[b], 16000, 22050))
    check_against_float64(x[1199:].cpu().numpy(), 16000, 22050)


# ---- 7. ragged equals alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", [(24000, 22050), (16000, 22050)])
def test_ragged_equals_each_utterance_alone(orig, new):
    lens = [4001, 2500, 161, 1]
    rs = np.random.RandomState(11)
    x = rs.standard_normal((4, 4001)).astype(np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = np.nan                                                # whatever lies behind an utterance must never be read
    xd = torch.from_numpy(x).cuda()
    y, n_out = audio_processing.resample_ragged(xd, lens, orig, new)
    assert n_out.dtype == torch.int64 and not n_out.is_cuda
    assert n_out.tolist() == [R.out_len(n, orig, new) for n in lens]
    assert y.shape == (4, max(n_out.tolist()))
    assert torch.isfinite(y).all()
    for b, n in enumerate(lens):
        alone = audio_processing.resample(xd[b, :n], orig, new)
        assert torch.equal(y[b, :n_out[b]], alone), b
        assert (y[b, n_out[b]:] == 0).all(), b
    y2, _ = audio_processing.resample_ragged(xd, torch.tensor(lens), orig, new)          # lengths as a CPU tensor
    assert torch.equal(y, y2)


# ---- 8. DC gain and impulse response -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", [(24000, 22050), (48000, 8000), (8000, 48000)])
def test_constant_and_impulse(orig, new):
    taps, start, og, ng, K = R.phase_table(orig, new)
    N = 1500
    c = np.float32(0.37)
    y = audio_processing.resample(torch.full((N,), float(c)).cuda(), orig, new).cpu().numpy().astype(np.float64)
    gain, mag = taps.sum(axis=1), np.abs(taps).sum(axis=1)
    m = np.arange(len(y))
    inside = slice(200, len(y) - 200)
    want, bound = float(c) * gain[m % ng], (K + 3) * EPS * float(c) * mag[m % ng]
    assert (np.abs(y - want)[inside] <= bound[inside]).all()
    taps32 = taps.astype(np.float32)
    for k0 in (0, 700, N - 1):
        x = torch.zeros(N)
        x[k0] = 1.0
        got = audio_processing.resample(x.cuda(), orig, new).cpu().numpy()
        want = np.zeros(len(got), dtype=np.float32)
        for mm in range(len(got)):
            q, p = divmod(mm, ng)
            i = k0 - q * og - int(start[p])
            if 0 <= i < K:
                want[mm] = taps32[p, i]
        assert np.count_nonzero(want) >= 5                               # half a window's worth of outputs even at the ends
        assert np.array_equal(got, want), k0


# ---- the data path -------------------------------------------------------------------------------------------------------------
RATES = [24000, 22050, 24000, 16000]


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    rows, counts = C.write_wavs(tmp_path_factory.mktemp("mixed_rates"), RATES)
    ds = Data(rows, text_frontend=C.grapheme_frontend, resample=True, **C.DATA_KW)
    items = [ds[i] for i in range(4)]
    return rows, counts, items


# ---- 9. launch count -----------------------------------------------------------------------------------------------------------
def test_launch_counts(mixed, monkeypatch):
    _, _, items = mixed
    batch = DataCollate(n_frames_per_step=1, use_attn_prior=True)(items)
    x = torch.randn(5, 3000).cuda()
    audio_processing.resample(x, 24000, 22050)                                           # table upload outside the count
    calls = count_calls(monkeypatch, ["ft_resample_ragged", "ft_stft_r8_ragged"])
    audio_processing.resample(x, 24000, 22050)
    assert calls == {"ft_resample_ragged": 1, "ft_stft_r8_ragged": 0}
    audio_processing.resample_ragged(x, [3000, 5, 17, 2999, 1], 24000, 22050)
    assert calls["ft_resample_ragged"] == 2
    batch[0].cuda()
    assert calls == {"ft_resample_ragged": 4, "ft_stft_r8_ragged": 1}                    # one per distinct source rate (24 k, 16 k)
    DataCollate()([items[1]])[0].cuda()                                                  # target rate only: no resampling launch
    assert calls == {"ft_resample_ragged": 4, "ft_stft_r8_ragged": 2}


# ---- 10. end to end ------------------------------------------------------------------------------------------------------------
def test_mixed_rate_batch_end_to_end(mixed):
    rows, counts, items = mixed
    batch = DataCollate(n_frames_per_step=1, use_attn_prior=True)(items)
    slot, out_lens = batch[0], batch[4]
    mel = slot.cuda()
    T = int(out_lens.max())
    assert mel.shape == (4, 80, T) and mel.is_cuda and torch.isfinite(mel).all()
    # by hand on the same audio: resample each source rate's rows, then one ragged front-end launch
    order = sorted(range(4), key=lambda i: -len(items[i][2]))
    audio = [items[i][0].audio.cuda() for i in order]
    rates = [RATES[i] for i in order]
    new_lens = [n if r == C.TARGET_SR else R.out_len(n, r, C.TARGET_SR) for n, r in zip([counts[i] for i in order], rates)]
    y = torch.zeros(4, max(new_lens)).cuda()
    for rate in (24000, 16000):
        idx = [i for i, r in enumerate(rates) if r == rate]
        n = [audio[i].numel() for i in idx]
        x = torch.zeros(len(idx), max(n)).cuda()
        for j, i in enumerate(idx):
            x[j, :n[j]] = audio[i]
        r, n_out = audio_processing.resample_ragged(x, n, rate, C.TARGET_SR)
        for j, i in enumerate(idx):
            assert int(n_out[j]) == new_lens[i]
            y[i, :new_lens[i]] = r[j, :new_lens[i]]
    same = rates.index(C.TARGET_SR)
    y[same, :new_lens[same]] = audio[same]
    stft = audio_processing.TacotronSTFT(1024, C.HOP, 1024, 80, C.TARGET_SR, 0.0, 8000.0).cuda()
    by_hand = stft.mel_spectrogram_ragged(y, torch.tensor(new_lens, dtype=torch.int32).cuda(), T)
    assert torch.equal(mel, by_hand)
    for i, n in enumerate(new_lens):
        assert out_lens[i] == n // C.HOP + 1
        assert (mel[i, :, n // C.HOP + 1:] == 0).all()
    # the file already at the target rate: what the data path without the switch gives for it alone
    plain = Data(rows, text_frontend=C.grapheme_frontend, **C.DATA_KW)
    alone = DataCollate()([plain[1]])[0].cuda()
    t = alone.shape[2]
    assert torch.equal(mel[same, :, :t], alone[0])


def test_one_training_step_from_a_mixed_rate_batch(mixed):
    import flowtron
    from oracle import synth
    _, _, items = mixed
    torch.manual_seed(0)
    cfg = dict(synth.SMALL_MODEL_CONFIG, n_hidden=128, n_attn_channels=64, n_speakers=1)
    model = flowtron.Flowtron(**cfg).cuda().train()
    crit = flowtron.FlowtronLoss(1.0, False, True, True, 0.01, -8)
    mel, spk, text, in_lens, out_lens, gate, prior = DataCollate(n_frames_per_step=1, use_attn_prior=True)(items)
    mel, spk, text, in_lens, out_lens, gate, prior = (t.cuda() for t in (mel, spk, text, in_lens, out_lens, gate, prior))
    out = model(mel, spk, text, in_lens, out_lens, prior)
    nll, gl, ctc = crit(out, gate, in_lens, out_lens)
    loss = nll + gl + 0.01 * ctc
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)


# ---- 11. equal rates, ABI ------------------------------------------------------------------------------------------------------
def test_equal_rates_and_abi(monkeypatch):
    calls = count_calls(monkeypatch, ["ft_resample_ragged"])
    x = torch.randn(3, 500).cuda()
    assert torch.equal(audio_processing.resample(x, 22050, 22050), x)
    assert torch.equal(audio_processing.resample(x[0], 8000, 8000), x[0])
    x[1, 200:] = float("nan")
    y, n_out = audio_processing.resample_ragged(x, [500, 200, 1], 22050, 22050)
    assert n_out.tolist() == [500, 200, 1] and torch.equal(y[1, :200], x[1, :200]) and (y[1, 200:] == 0).all()
    assert torch.equal(y[0], x[0]) and (y[2, 1:] == 0).all()
    assert calls["ft_resample_ragged"] == 0
    h = ctypes.CDLL(L.LIB_PATH)
    assert h.ft_abi_version() == 15
    assert hasattr(h, "ft_resample_ragged") and hasattr(h, "ft_resample_out_len")
    # the C entry refuses a table it cannot hold, with a message, before any launch
    rc = L.lib().ft_resample_ragged(L.ptr(x), None, L.ptr(x), L.ptr(x), L.ptr(x), 1, 500, 500, 22050, 22051, 13, L.stream())
    assert rc == -3 and b"phases" in L.lib().ft_last_error()
