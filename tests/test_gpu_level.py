"""Endpoints and loudness on the device (-m gpu): the kernels of csrc/level.hip against their NumPy replay (tests/level_ref.py) bit
for bit -- frame powers, bounds, peak, step sums, gated power, gain and the gathered output, for every utterance alone and in a
batch whose padding is NaN --, loudness of a span in place against loudness of the trimmed batch, prepare against the
composition of its steps, the mel front end on prepare's output, the level after normalize, and the corpus pass as a child
process.  8000 Hz: a step of 800 samples, a block of 3200, frames of 256 samples every 64."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import level_ref as R
from call_count import count_calls
from flowtron_amd import level
from flowtron_amd.audio import TacotronSTFT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, F, HOP, N = 8000, 256, 64, 16077
STEP = SR // 10
KW = dict(top_db=60.0, frame_length=F, hop_length=HOP)
LENGTHS = (16077, 6400, 3200, 3199, 257)          # full row; whole steps and chunks; one block; no block; one chunk and a sample

_CASES = {}


def utterances(which):
    if which == "batch":
        quiet = R.voice(6400, SR, 640, 6400, seed=1, amplitude=0.003)         # wants more than max_gain_db
        return [R.voice(16077, SR, 4000, 12877, seed=0), quiet, R.tone(3200, SR, 997.0, 0.5), R.voice(3199, SR, 0, 3199, seed=2),
                R.tone(257, SR, 440.0, 0.25)]
    click = R.voice(9000, SR, 1000, 8000, seed=4, amplitude=0.05)
    click[5000] = np.float32(0.9)                                             # the peak ceiling binds
    return [click]


def case(which):
    """the utterances, their NaN-padded batch and every replayed result, made once"""
    if which not in _CASES:
        xs = utterances(which)
        n_max = N if which == "batch" else len(xs[0])
        X = np.full((len(xs), n_max), np.nan, np.float32)
        for b, x in enumerate(xs):
            X[b, :len(x)] = x
        rep = []
        for x in xs:
            power = R.frame_powers(x, F, HOP)
            lufs, gated, sums = R.loudness(x, SR)
            rep.append(dict(power=power, bounds=R.bounds(power, len(x), HOP, 60.0), peak=R.peak(x), lufs=lufs, gated=gated, sums=sums,
                            prepared=R.prepare(x, n_max, SR, frame_length=F, hop=HOP)))
        _CASES[which] = (xs, X, [len(x) for x in xs], rep)
    return _CASES[which]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.tobytes()


def same64(a, b):
    """float64 values with the same bits, any NaN equal to any NaN"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def test_the_batch_holds_what_it_is_meant_to_hold():
    xs, X, lens, rep = case("batch")
    assert tuple(lens) == LENGTHS and X.shape == (5, N) and np.isnan(X[1, 6400:]).all()
    assert rep[0]["bounds"] == (3904, 13056) and rep[1]["bounds"][0] > 0 and rep[2]["bounds"] == (0, 3200)
    assert [len(r["sums"]) for r in rep] == [20, 8, 4, 3, 0]
    assert math_isnan(rep[3]["gated"]) and math_isnan(rep[4]["gated"]) and all(r["gated"] > 0 for r in rep[:3])
    gains = [float(r["prepared"]["gain"]) for r in rep]
    assert gains[1] == float(np.float32(10.0 ** 1.5)) and gains[3] == 1.0 and gains[4] == 1.0 and gains[2] < 1.0      # the cap binds once
    assert float(case("single")[3][0]["prepared"]["gain"]) == float(np.float32(0.99 / float(np.float32(0.9))))    # and the ceiling


def math_isnan(v):
    return v != v


@pytest.mark.parametrize("which", ["batch", "single"])
def test_powers_bounds_and_peak_equal_the_replay_alone_and_in_the_batch(which):
    xs, X, lens, rep = case(which)
    got = level.active_bounds(dev(X), lens, return_all=True, **KW)
    from_dev = level.active_bounds(dev(X), torch.tensor(lens, dtype=torch.int32).cuda(), return_all=True, **KW)
    assert got.power.dtype == torch.float32 and got.start.dtype == torch.int32 and got.end.dtype == torch.int32 and got.start.is_cuda
    assert tuple(got.power.shape) == (len(xs), X.shape[1] // HOP + 1)
    assert all(bits(a) == bits(b) for a, b in zip(got, from_dev))            # a host and a device length vector
    contour = level.frame_power(dev(X), lens, F, HOP)
    assert bits(contour) == bits(got.power)
    power, start, end, pk = got.power.cpu().numpy(), got.start.tolist(), got.end.tolist(), got.peak.cpu().numpy()
    for b, (x, r) in enumerate(zip(xs, rep)):
        T = len(x) // HOP + 1
        assert power[b, :T].tobytes() == r["power"].tobytes(), b
        assert not power[b, T:].any()
        assert (start[b], end[b]) == r["bounds"], b
        assert pk[b].tobytes() == r["peak"].tobytes(), b
        alone = level.active_bounds(dev(x), None, return_all=True, **KW)
        assert alone.start.dim() == 0 and bits(alone.power) == r["power"].tobytes()
        assert (int(alone.start), int(alone.end)) == r["bounds"] and bits(alone.peak) == r["peak"].tobytes()
    s, e = level.active_bounds(dev(X), lens, pad=100, **KW)
    assert s.tolist() == [max(r["bounds"][0] - 100, 0) for r in rep]
    assert e.tolist() == [min(r["bounds"][1] + 100, n) for r, n in zip(rep, lens)]


@pytest.mark.parametrize("which", ["batch", "single"])
def test_step_sums_and_gated_power_equal_the_replay_alone_and_in_the_batch(which):
    xs, X, lens, rep = case(which)
    got = level.loudness(dev(X), lens, SR, return_all=True)
    from_dev = level.loudness(dev(X), torch.tensor(lens, dtype=torch.int32).cuda(), SR, return_all=True)
    assert got.power.dtype == torch.float64 and got.lufs.dtype == torch.float64 and got.lufs.is_cuda
    assert tuple(got.step_sums.shape) == (len(xs), X.shape[1] // STEP)
    assert same64(got.power.cpu().numpy(), from_dev.power.cpu().numpy()) and bits(got.step_sums) == bits(from_dev.step_sums)
    sums, power, lufs = got.step_sums.cpu().numpy(), got.power.cpu().numpy(), got.lufs.cpu().numpy()
    for b, (x, r) in enumerate(zip(xs, rep)):
        ns = len(r["sums"])
        assert sums[b, :ns].tobytes() == r["sums"].tobytes(), b
        assert not sums[b, ns:].any()
        assert same64(power[b], r["gated"]), (b, power[b], r["gated"])
        if np.isfinite(r["lufs"]):
            print("utterance %d: %.6f LUFS on the device, %.6f replayed" % (b, lufs[b], r["lufs"]))
            assert abs(lufs[b] - r["lufs"]) <= 1e-12 * abs(r["lufs"])
        else:
            assert np.isnan(lufs[b])
        assert bits(got.peak[b]) == r["peak"].tobytes()
        alone = level.loudness(dev(x), None, SR, return_all=True)
        assert same64(alone.power.cpu().numpy(), r["gated"]) and bits(alone.step_sums[:ns]) == r["sums"].tobytes()
    lufs2, power2 = level.loudness(dev(X), lens, SR)
    assert same64(power2.cpu().numpy(), power) and same64(lufs2.cpu().numpy(), lufs)


def test_loudness_of_a_span_in_place_equals_loudness_of_the_trimmed_batch():
    xs, X, lens, rep = case("batch")
    x = dev(X)
    start, end = level.active_bounds(x, lens, **KW)
    trimmed, n_out = level.trim(x, lens, **KW)
    assert n_out.dtype == torch.int32 and n_out.is_cuda and n_out.tolist() == [r["bounds"][1] - r["bounds"][0] for r in rep]
    t = trimmed.cpu().numpy()
    for b, (xb, r) in enumerate(zip(xs, rep)):
        assert t[b].tobytes() == R.gather(xb, r["bounds"][0], r["bounds"][1], N).tobytes(), b
    in_place = level.loudness(x, lens, SR, start=start, end=end, return_all=True)
    of_trimmed = level.loudness(trimmed, n_out, SR, return_all=True)
    assert same64(in_place.power.cpu().numpy(), of_trimmed.power.cpu().numpy())
    assert bits(in_place.step_sums) == bits(of_trimmed.step_sums) and bits(in_place.peak) == bits(of_trimmed.peak)
    assert same64(in_place.lufs.cpu().numpy(), of_trimmed.lufs.cpu().numpy())
    for b, r in enumerate(rep):
        assert same64(in_place.power[b].item(), r["prepared"]["power"]), b


@pytest.mark.parametrize("which", ["batch", "single"])
def test_prepare_equals_its_steps_and_the_replay(which, monkeypatch):
    xs, X, lens, rep = case(which)
    x = dev(X)
    entries = ("ft_level_bounds", "ft_level_loudness", "ft_level_gather")
    calls = count_calls(monkeypatch, entries)
    out, n_out, info = level.prepare(x, lens, SR, **KW)
    assert calls == {n: 1 for n in entries}                                  # seven launches behind three entries
    trimmed, n_trim = level.trim(x, lens, **KW)
    ld = level.loudness(trimmed, n_trim, SR, return_all=True)
    gain = level.gain_for(ld.lufs, ld.peak)
    again, n_again = level.trim(x, lens, gain=gain, **KW)
    assert bits(out) == bits(again) and bits(n_out) == bits(n_again) == bits(n_trim) and bits(info.gain) == bits(gain)
    assert same64(info.lufs.cpu().numpy(), ld.lufs.cpu().numpy()) and bits(info.peak) == bits(ld.peak)
    o, g = out.cpu().numpy(), info.gain.cpu().numpy()
    for b, r in enumerate(rep):
        p = r["prepared"]
        assert (int(info.start[b]), int(info.end[b]), int(n_out[b])) == (p["start"], p["end"], p["n_out"]), b
        assert g[b].tobytes() == p["gain"].tobytes(), (b, g[b], p["gain"])
        assert bits(info.peak[b]) == p["peak"].tobytes()
        assert o[b].tobytes() == p["out"].tobytes(), b
        alone = level.prepare(dev(xs[b]), None, SR, **KW)
        assert bits(alone[0]) == p["out"][:len(xs[b])].tobytes() and int(alone[1]) == p["n_out"]


def test_mel_front_end_takes_prepares_output_and_device_lengths():
    xs, X, lens, rep = case("batch")
    out, n_out, _ = level.prepare(dev(X), lens, SR, **KW)
    stft = TacotronSTFT(filter_length=256, hop_length=64, win_length=256, n_mel_channels=40, sampling_rate=SR, mel_fmin=0.0,
                        mel_fmax=4000.0).cuda()
    mel = stft.mel_spectrogram_ragged(out, n_out)
    for b, n in enumerate(n_out.tolist()):
        alone = stft.mel_spectrogram(out[b:b + 1, :n].contiguous())
        T = n // 64 + 1
        assert tuple(alone.shape) == (1, 40, T)
        assert bits(mel[b, :, :T]) == bits(alone[0]), b


def test_normalized_utterances_measure_at_the_target():
    xs, X, lens, rep = case("batch")
    out, gain = level.normalize(dev(X), lens, SR, target_lufs=-23.0, peak_ceiling=None, max_gain_db=60.0)
    o, g = out.cpu().numpy(), gain.cpu().numpy()
    for b, (x, r) in enumerate(zip(xs, rep)):
        want = R.gain_for(r["lufs"], r["peak"], -23.0, None, 60.0)
        assert g[b].tobytes() == want.tobytes(), (b, g[b], want)
        assert o[b].tobytes() == R.gather(x, 0, len(x), N, want).tobytes(), b
        if len(r["sums"]) >= 4:
            again = R.loudness(o[b, :len(x)], SR)[0]
            print("utterance %d: %.4f LUFS before, gain %.4f, %.4f LUFS after" % (b, r["lufs"], g[b], again))
            assert abs(again - (-23.0)) <= 0.05
    peak_only, gp = level.normalize(dev(X), lens, SR, target_lufs=None, peak_ceiling=0.5, max_gain_db=60.0)
    for b, (x, r) in enumerate(zip(xs, rep)):
        want = R.gain_for(float("nan"), r["peak"], None, 0.5, 60.0)
        assert bits(gp[b]) == want.tobytes() and bits(peak_only[b]) == R.gather(x, 0, len(x), N, want).tobytes()


def test_digital_silence_keeps_its_length_and_a_gain_of_one():
    x = dev(R.silence(4000))
    out, n_out, info = level.prepare(x, None, SR, **KW)
    assert (int(info.start), int(info.end), int(n_out)) == (0, 4000, 4000)
    assert float(info.lufs) == float("-inf") and float(info.gain) == 1.0 and float(info.peak) == 0.0 and not out.any()
    lufs, power = level.loudness(x[:3199], None, SR)
    assert np.isnan(float(lufs)) and np.isnan(float(power))


def write_wav(path, x, sr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.round(np.clip(x.astype(np.float64), -1, 1) * 32767.0).astype("<i2").tobytes())


def test_corpus_pass_writes_wavs_filelist_and_report(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    items = [("a.wav", R.voice(12000, 8000, 3000, 10000, seed=5), 8000, "first sentence.", "0"),
             ("b.wav", R.voice(16000, 16000, 4000, 13000, seed=6), 16000, "second one, at another rate.", "3"),
             ("c.wav", R.voice(9000, 8000, 0, 9000, seed=7, amplitude=0.05), 8000, "third.", "1")]
    for name, x, sr, _, _ in items:
        write_wav(src / name, x, sr)
    filelist = tmp_path / "in.txt"
    filelist.write_text("".join("%s|%s|%s\n" % (src / name, text, spk) for name, _, _, text, spk in items), encoding="utf-8")
    out_dir, out_list = tmp_path / "out", tmp_path / "out.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "prepare_corpus.py"), "--filelist", str(filelist), "--out-dir", str(out_dir),
                        "--out-filelist", str(out_list), "--sampling-rate", "8000", "--frame-length", "256", "--hop-length", "64",
                        "--batch", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split("|") for l in out_list.read_text(encoding="utf-8").splitlines()]
    assert [(l[1], l[2]) for l in lines] == [(text, spk) for _, _, _, text, spk in items]
    report = [json.loads(l) for l in (out_dir / "report.jsonl").read_text().splitlines()]
    assert len(report) == 3 and [os.path.basename(j["path"]) for j in report] == ["a.wav", "b.wav", "c.wav"]
    for (path, _, _), j in zip(lines, report):
        assert path == j["path"] and os.path.dirname(path) == str(out_dir)
        with wave.open(path, "rb") as w:
            assert w.getframerate() == 8000 and w.getnchannels() == 1 and w.getsampwidth() == 2
            assert w.getnframes() == j["end"] - j["start"] == j["n_out"] > 0
            pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2")
        assert abs(np.abs(pcm).max() / 32767.0 - j["peak_after"]) <= 2.0 / 32767.0
        assert set(j) >= {"start", "end", "lufs_before", "gain", "peak_after"}
    assert report[0]["start"] > 2000 and report[0]["end"] < 11000            # the silence is gone
    assert report[1]["orig_sampling_rate"] == 16000 and 1500 < report[1]["start"] <= 2000
    assert abs(report[0]["lufs_before"] + 20.0 * np.log10(report[0]["gain"]) - (-23.0)) <= 0.01
