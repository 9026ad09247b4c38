"""Endpoints and loudness without a GPU: the host tables of flowtron_amd.level against the standard's printed 48 kHz table, the
NumPy replay of the kernels (tests/level_ref.py) against the standard's 997 Hz levels and against scipy.signal.lfilter in
float64, the endpoint rule on a signal of known onset and offset, the edge cases of loudness and gain, and the refusals of the
Python layer and of the C entries of csrc/level.hip before anything reaches the device."""
import math

import numpy as np
import pytest
import torch

import level_ref as R
from flowtron_amd import level

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
SHELF_B = (1.53512485958697, -2.69169618940638, 1.19839281085285)
SHELF_A = (1.0, -1.69065929318241, 0.73248077421585)
HIGHPASS_B = (1.0, -2.0, 1.0)
HIGHPASS_A = (1.0, -1.99004745483398, 0.99007225036621)


def test_coefficients_equal_the_standards_table_at_48_khz():
    sb, sa, hb, ha = level.k_weighting(48000)
    worst = max(abs(g - w) for got, want in ((sb, SHELF_B), (sa, SHELF_A), (hb, HIGHPASS_B), (ha, HIGHPASS_A)) for g, w in zip(got, want))
    print("largest difference to the printed table: %.2e" % worst)
    assert worst <= 1e-12
    assert level.filter_coefficients(48000) == (sb[0], sb[1], sb[2], sa[1], sa[2], ha[1], ha[2])
    assert level.block_step(11025) * 4 == 4408 and level.block_step(22050) == 2205


def test_full_scale_997_hz_sine_is_minus_3_01_lufs():
    lufs, power, _ = R.loudness(R.tone(3 * 48000, 48000), 48000)
    print("full-scale 997 Hz, 3 s at 48 kHz: %.4f LUFS" % lufs)
    assert abs(lufs - (-3.01)) <= 0.01


def test_minus_20_dbfs_sine_is_minus_23_01_lufs():
    lufs, _, _ = R.loudness(R.tone(20 * 48000, 48000, amplitude=0.1), 48000)
    print("-20 dBFS 997 Hz, 20 s at 48 kHz: %.4f LUFS" % lufs)
    assert abs(lufs - (-23.01)) <= 0.01


def test_relative_gate_removes_the_quiet_half():
    x = R.tone(20 * 48000, 48000, amplitude=0.1)
    x[10 * 48000:] *= np.float32(10.0 ** (-30.0 / 20.0))                    # -50 dBFS
    lufs, _, _ = R.loudness(x, 48000)
    print("10 s at -20 dBFS then 10 s at -50 dBFS: %.4f LUFS (ungated mean -26.0)" % lufs)
    assert abs(lufs - (-23.01)) <= 0.1
    assert lufs > -26.0 + 2.0


@pytest.mark.parametrize("sr", [8000, 22050, 48000])
@pytest.mark.parametrize("chunk", [64, 256])
def test_three_pass_filter_equals_scipy_lfilter(sr, chunk):
    signal = pytest.importorskip("scipy.signal")
    assert level.CHUNK == 256                                               # the kernel's chunk length is among the cases
    n = 2 * sr + 77
    x = R.voice(n, sr, sr // 2, n - sr // 3, seed=3)
    sb, sa, hb, ha = level.k_weighting(sr)
    want = signal.lfilter(hb, ha, signal.lfilter(sb, sa, x.astype(np.float64)))
    got = R.k_filter(x, sr, chunk)
    rel = math.sqrt(float(np.sum((got - want) ** 2)) / float(np.sum(want ** 2)))
    print("sr %d, chunk %d: relative rms to scipy.signal.lfilter %.2e" % (sr, chunk, rel))
    assert rel <= 1e-10


def test_chunk_length_does_not_change_the_loudness_beyond_rounding():
    x = R.voice(16077, 8000, 4000, 12877)
    a, b = R.loudness(x, 8000, 256)[1], R.loudness(x, 8000, 64)[1]
    assert abs(a / b - 1) <= 1e-10


@pytest.mark.parametrize("top_db", [40.0, 60.0])
def test_endpoints_of_a_voice_with_an_80_db_step(top_db):
    F, hop, onset, offset = 256, 64, 4000, 12877
    x = R.voice(16077, 8000, onset, offset)
    s, e = R.active_bounds(x, top_db, F, hop)
    print("top_db %g: start %d for an onset at %d, end %d for an offset at %d" % (top_db, s, onset, e, offset))
    assert onset - (F // 2 + hop) <= s <= onset
    assert offset <= e <= offset + F // 2 + hop
    assert s % hop == 0 and e % hop == 0
    assert R.active_bounds(x, top_db, F, hop, pad=100) == (s - 100, e + 100)
    assert R.active_bounds(x, top_db, F, hop, pad=10 ** 6) == (0, 16077)


def test_endpoints_keep_an_utterance_without_silence_and_digital_silence():
    F, hop = 256, 64
    x = R.voice(6000, 8000, 0, 6000)
    s, e = R.active_bounds(x, 60.0, F, hop)
    assert s == 0 and 6000 - hop < e <= 6000
    assert R.active_bounds(R.silence(6000), 60.0, F, hop) == (0, 6000)
    assert R.active_bounds(x, 60.0, F, hop, ref=1.0e6) == (0, 6000)          # nothing above an absolute reference
    assert R.active_bounds(np.ones(1, np.float32), 60.0, F, hop) == (0, 1)
    p = R.frame_powers(x, F, hop)
    assert p.dtype == np.float32 and p.shape == (6000 // hop + 1,)
    inner = np.array([np.mean(x[t * hop - F // 2:t * hop + F // 2].astype(np.float64) ** 2) for t in range(2, 90)])
    assert np.max(np.abs(p[2:90] / inner - 1)) <= 2.0 ** -23                 # one fp32 rounding of a float64 mean


def test_loudness_edge_cases_and_the_gain_rule():
    sr, step = 8000, 800
    x = R.voice(4 * step, sr, 0, 4 * step)
    lufs_short, power_short, sums = R.loudness(x[:4 * step - 1], sr)
    assert math.isnan(lufs_short) and math.isnan(power_short) and len(sums) == 3
    assert R.gain_for(lufs_short, R.peak(x)) == np.float32(1)
    lufs_one, power_one, sums = R.loudness(x, sr)
    assert len(sums) == 4 and power_one == ((sums[0] + sums[1]) + (sums[2] + sums[3])) / 3200.0 and math.isfinite(lufs_one)
    lufs_sil, power_sil, _ = R.loudness(R.silence(8000), sr)
    assert power_sil == 0.0 and lufs_sil == float("-inf")
    assert R.gain_for(lufs_sil, 0.0) == np.float32(1)
    # plain case, then each limit binding in a case of its own
    assert R.gain_for(-33.0, 0.01) == np.float32(10.0 ** 0.5)
    assert R.gain_for(-33.0, 0.5) == np.float32(0.99 / 0.5)                  # the ceiling binds
    assert R.gain_for(-33.0, 0.5, peak_ceiling=None) == np.float32(10.0 ** 0.5)
    assert R.gain_for(-63.0, 1e-4) == np.float32(10.0 ** 1.5)                # max_gain_db binds: 40 dB wanted, 30 given
    assert R.gain_for(-63.0, 1e-4, max_gain_db=50.0) == np.float32(100.0)
    assert R.gain_for(float("nan"), 0.5, target_lufs=None) == np.float32(0.99 / 0.5)     # peak normalisation alone
    assert R.gain_for(float("nan"), 0.0, target_lufs=None) == np.float32(1)
    # flowtron_amd.level.gain_for is plain torch: the same values on the host
    lufs = torch.tensor([-33.0, -33.0, -63.0, float("nan"), float("-inf")], dtype=torch.float64)
    pk = torch.tensor([0.01, 0.5, 1e-4, 0.5, 0.0], dtype=torch.float32)
    got = level.gain_for(lufs, pk)
    want = [R.gain_for(float(l), float(p)) for l, p in zip(lufs.tolist(), pk.tolist())]
    assert got.dtype == torch.float32 and got.tolist() == [float(w) for w in want]
    got = level.gain_for(lufs, pk, target_lufs=None)
    assert got.tolist() == [float(R.gain_for(float("nan"), float(p), target_lufs=None)) for p in pk.tolist()]


def test_gather_replay_rounds_once():
    x = R.voice(1000, 8000, 100, 900)
    g = np.float32(1.2345678)
    out = R.gather(x, 64, 960, 1000, g)
    assert out.dtype == np.float32 and np.all(out[896:] == 0)
    assert np.array_equal(out[:896], (g.astype(np.float64) * x[64:960].astype(np.float64)).astype(np.float32))
    assert np.array_equal(R.gather(x, 64, 960, 1000)[:896], x[64:960])


def test_refusals_are_raised_without_a_device():
    x = torch.zeros(2, 8000)
    calls = (level.active_bounds, level.trim, level.frame_power, level.loudness, level.normalize, level.prepare)
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x)
        for bad in (x.double(), x[None], torch.zeros(2, 0), [0.0] * 10):
            with pytest.raises(ValueError, match="audio"):
                f(bad)
        for ns in ([8000], [8000, 8001], [8000, 0], torch.tensor([8000.0, 1.0])):
            with pytest.raises(ValueError, match="n_samples"):
                f(x, ns)
        with pytest.raises(NotImplementedError, match="65535"):
            f(torch.zeros(65536, 1))
    for f in (level.active_bounds, level.trim, level.prepare):
        for kw, what in ((dict(top_db=0.0), "top_db"), (dict(top_db=float("nan")), "top_db"), (dict(top_db=None), "top_db"),
                         (dict(frame_length=255), "even"), (dict(frame_length=0), "frame_length"), (dict(frame_length=256.0), "frame_length"),
                         (dict(hop_length=0), "hop_length"), (dict(frame_length=256, hop_length=257), "hop_length must not exceed"),
                         (dict(ref="mean"), "ref"), (dict(ref=0.0), "ref"), (dict(ref=-1.0), "ref"), (dict(pad=-1), "pad"), (dict(pad=1.5), "pad")):
            with pytest.raises(ValueError, match=what):
                f(x, **kw)
        with pytest.raises(NotImplementedError, match="4096"):
            f(x, frame_length=4098)
    with pytest.raises(ValueError, match="frame_length"):
        level.frame_power(x, frame_length=3)
    for f in (level.loudness, level.normalize, level.prepare):
        for sr in (0, 22050.0, None, True):
            with pytest.raises(ValueError, match="sampling_rate"):
                f(x, None, sr)
        with pytest.raises(NotImplementedError, match="2560"):
            f(x, None, 2559)
        with pytest.raises(NotImplementedError, match="4096"):
            f(torch.zeros(1, 4097 * 800), None, 8000)
    for f in (level.normalize, level.prepare):
        for kw, what in ((dict(target_lufs=float("inf")), "target_lufs"), (dict(target_lufs="loud"), "target_lufs"),
                         (dict(peak_ceiling=0.0), "peak_ceiling"), (dict(max_gain_db=float("nan")), "max_gain_db")):
            with pytest.raises(ValueError, match=what):
                f(x, None, 8000, **kw)
    for kw in (dict(start=[0, 0]), dict(start=torch.zeros(2, dtype=torch.int32)), dict(end=torch.zeros(2))):
        with pytest.raises(ValueError, match="int32 tensor on the device"):
            level.loudness(x, None, 8000, **kw)
    for g in ([1.0, 1.0], torch.ones(3), torch.ones(2, dtype=torch.float64)):
        with pytest.raises(ValueError, match="gain"):
            level.trim(x, gain=g)


def test_audio_processing_re_exports_the_public_calls():
    import audio_processing
    for name in ("active_bounds", "frame_power", "trim", "loudness", "normalize", "prepare"):
        assert getattr(audio_processing, name) is getattr(level, name)


def test_c_abi_refuses_bad_arguments_before_the_device():
    """FT_EINVAL / FT_EUNSUPPORTED from the entry points themselves, with host memory standing in for the buffers: nothing may
    be launched"""
    import ctypes as C
    from flowtron_amd import _lib as L
    lib = L.lib()
    assert lib.ft_abi_version() == 15
    B, N = 2, 1024
    audio = (C.c_float * (B * N))()
    n = (C.c_int32 * B)()
    f32 = [(C.c_float * (B * N))() for _ in range(4)]
    i32 = [(C.c_int32 * B)() for _ in range(3)]
    f64 = [(C.c_double * 64)() for _ in range(2)]
    coef = (C.c_double * 7)(*level.filter_coefficients(8000))
    M = level.carry_matrix(level.filter_coefficients(8000))
    carry = (C.c_double * 16)(*[M[r][j] for r in range(4) for j in range(4)])
    nbytes = lib.ft_level_loudness_workspace_bytes(B, N)
    assert nbytes == B * 4 * (10 * 8 + 4) and lib.ft_level_loudness_workspace_bytes(0, N) == 0 and lib.ft_level_loudness_workspace_bytes(B, 0) == 0
    work = (C.c_double * (nbytes // 8 + 1))()
    adr = C.addressof

    okb = dict(audio=adr(audio), s=(N, 1), n=adr(n), power=adr(f32[0]), fpeak=adr(f32[1]), peak=adr(f32[2]), start=adr(i32[0]),
               end=adr(i32[1]), B=B, N=N, F=256, hop=64, thr=1e-6, ref=0.0, pad=0)

    def bounds(**kw):
        a = dict(okb, **kw)
        return lib.ft_level_bounds(a["audio"], *a["s"], a["n"], a["power"], a["fpeak"], a["peak"], a["start"], a["end"], a["B"], a["N"],
                                   a["F"], a["hop"], a["thr"], a["ref"], a["pad"], None)
    for kw in (dict(audio=None), dict(n=None), dict(power=None), dict(fpeak=None), dict(peak=None), dict(start=None), dict(end=None),
               dict(B=0), dict(B=-1), dict(B=65536), dict(N=0), dict(F=255), dict(F=0), dict(F=1), dict(hop=0), dict(hop=257),
               dict(s=(-N, 1)), dict(s=(N, -1)), dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(ref=-1.0),
               dict(ref=float("nan")), dict(pad=-1)):
        assert bounds(**kw) == -1, kw
        assert b"ft_level_bounds" in lib.ft_last_error()
    assert bounds(F=4098) == -3 and b"4096" in lib.ft_last_error()

    okl = dict(audio=adr(audio), s=(N, 1), n=adr(n), start=None, end=None, coef=coef, carry=carry, gate=level.absolute_gate_power(),
               sums=adr(f64[0]), power=adr(f64[1]), peak=adr(f32[2]), work=adr(work), wb=nbytes, B=B, N=N, step=800)

    def loud(**kw):
        a = dict(okl, **kw)
        return lib.ft_level_loudness(a["audio"], *a["s"], a["n"], a["start"], a["end"], a["coef"], a["carry"], a["gate"], a["sums"],
                                     a["power"], a["peak"], a["work"], a["wb"], a["B"], a["N"], a["step"], None)
    bad_coef = (C.c_double * 7)(*([float("nan")] + list(coef)[1:]))
    bad_carry = (C.c_double * 16)(*([float("inf")] + list(carry)[1:]))
    for kw in (dict(audio=None), dict(n=None), dict(coef=None), dict(carry=None), dict(sums=None), dict(power=None), dict(peak=None),
               dict(work=None), dict(B=0), dict(B=65536), dict(N=0), dict(step=0), dict(step=-800), dict(s=(-N, 1)), dict(s=(N, -1)),
               dict(gate=-1.0), dict(gate=float("nan")), dict(wb=nbytes - 1), dict(work=adr(work) + 4), dict(coef=bad_coef),
               dict(carry=bad_carry)):
        assert loud(**kw) == -1, kw
        assert b"ft_level_loudness" in lib.ft_last_error()
    for kw in (dict(step=255), dict(step=1)):                                # FT_EUNSUPPORTED: a step shorter than a chunk
        assert loud(**kw) == -3, kw
        assert b"256" in lib.ft_last_error() and b"4096" in lib.ft_last_error()

    okg = dict(audio=adr(audio), s=(N, 1), n=adr(n), start=None, end=None, gain=None, out=adr(f32[3]), n_out=adr(i32[2]), B=B, N=N)

    def gather(**kw):
        a = dict(okg, **kw)
        return lib.ft_level_gather(a["audio"], *a["s"], a["n"], a["start"], a["end"], a["gain"], a["out"], a["n_out"], a["B"], a["N"], None)
    for kw in (dict(audio=None), dict(n=None), dict(out=None), dict(n_out=None), dict(B=0), dict(B=65536), dict(N=0), dict(s=(-N, 1)),
               dict(s=(N, -1))):
        assert gather(**kw) == -1, kw
        assert b"ft_level_gather" in lib.ft_last_error()
