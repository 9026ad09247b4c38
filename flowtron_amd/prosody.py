"""Pitch and pace of audio on the device: time-domain pitch-synchronous overlap-add (TD-PSOLA) on the F0 track (additive: the
reference has no F0 input and no way to change the pitch; csrc/prosody.hip).

    audio = stft.mel_to_audio_ragged(mel, lengths)                               # or a recording
    audio, n = level.trim(audio, n_samples)
    f0, _ = pitch.f0_track(audio, n, hop_length=hop)                             # [B, T] Hz, 0 = unvoiced
    ratio = prosody.pitch_ratio(f0, shift_semitones=3.0, range_scale=0.5)        # [B, T]: three semitones up, half the range
    out, n_out = prosody.modify(audio, n, f0, hop_length=hop, pitch_ratio=ratio, pace=1.1)
    mel = stft.mel_spectrogram_ragged(out, n_out)                                # n_out is an int32 tensor on the device

Two-period Hann grains are cut at analysis marks one F0 period apart (integrated from the track: no search for glottal pulses)
and laid down again at synthesis marks period / ratio apart, each taking the grain whose analysis mark is nearest in the
input's time: the fundamental moves, the spectral envelope stays, and pace moves along the input faster or slower without
re-synthesis.  Positions are integers in 1/256 sample, the window a host-made table, every fp32 operation rounded on its own:
include/flowtron_hip.h states the rule and tests/prosody_ref.py replays it bit for bit.  Every utterance gives the same bits
alone as in any batch; nothing here synchronises with the host.  What the tests pin is F0, envelope, length and bits, not how
it sounds; no outside PSOLA implementation was available to compare with.

A pace that varies within the utterance -- the rhythm and melody of a recording, or one word slowed down -- is warp() along a
time map (time_map_from_path, time_map_from_durations) with transfer_ratio for the melody: further down, with its own example."""
from __future__ import annotations

import collections
import math
import numbers

import numpy as np
import torch

from . import _lib as L
from .level import _audio_arg, _int_arg, _lengths

Q = 256                    # FT_PSOLA_Q: positions are integers in 1 / Q sample
MIN_RATIO, MAX_RATIO = 0.625, 2.0          # below 0.625 neighbouring two-period grains stop overlapping (0.19 between marks there)
MIN_PACE, MAX_PACE = 0.25, 4.0
MIN_PERIOD, MAX_PERIOD = 16, 1024          # FT_PSOLA_MIN_PERIOD / FT_PSOLA_MAX_PERIOD, samples
MAX_SAMPLES = 1 << 22      # FT_PSOLA_MAX_SAMPLES: N and N_out (positions stay below 2^31)
MAX_BATCH = 65535
HANN_STEPS = 1024          # FT_PSOLA_HANN: the window table holds HANN_STEPS + 1 values

Marks = collections.namedtuple("Marks", "analysis n_analysis synthesis source half n_synthesis n_out")


# ---- host pieces (tests/prosody_ref.py uses these very functions) ---------------------------------------------------------------

def hann_table():
    """-> [1025] float64: 0.5 + 0.5 cos(pi i / 1024), the falling half of the window; the kernels take it rounded once to fp32"""
    return 0.5 + 0.5 * np.cos(np.pi * np.arange(HANN_STEPS + 1, dtype=np.float64) / HANN_STEPS)


def pace_q(pace):
    """the pace in 1 / 65536: the nearest integer, halves to even"""
    return int(round(float(pace) * 65536.0))


def default_unvoiced_period(sampling_rate):
    """the grain spacing where nothing is voiced: 5 ms"""
    return int(round(float(sampling_rate) / 200.0))


def out_samples(n, pace):
    """the samples of an utterance of n at this pace: max(1, (n << 16) // pace_q(pace))"""
    return max(1, (int(n) << 16) // pace_q(pace))


# ---- argument checks ----------------------------------------------------------------------------------------------------------------

def _args(who, audio, n_samples, f0, sampling_rate, hop_length, pitch_ratio, pace, unvoiced_period):
    a2, single = _audio_arg(audio, who)
    B, N = a2.shape
    if isinstance(sampling_rate, bool) or not isinstance(sampling_rate, numbers.Real) or not math.isfinite(sampling_rate) or sampling_rate <= 0:
        raise ValueError("sampling_rate must be a positive number, got %r" % (sampling_rate,))
    sr256 = float(np.float32(float(sampling_rate) * 256.0))
    if isinstance(hop_length, bool) or not isinstance(hop_length, numbers.Integral) or hop_length < 1:
        raise ValueError("hop_length must be an integer >= 1, got %r" % (hop_length,))
    hop = int(hop_length)
    if not torch.is_tensor(f0) or f0.dtype != torch.float32 or f0.dim() != a2.dim() - (1 if single else 0) or \
            (f0[None] if single else f0).shape[0] != B:
        raise ValueError("f0 must be a float32 %s tensor as pitch.f0_track returns it, got %s"
                         % ("[T]" if single else "[%d, T]" % B, (tuple(f0.shape), f0.dtype) if torch.is_tensor(f0) else type(f0).__name__))
    f2 = (f0[None] if single else f0).detach()
    T = f2.shape[1]
    if T < N // hop + 1:
        raise ValueError("f0 must hold at least N // hop_length + 1 = %d frames (frame t is centred on sample t * hop_length), got %d"
                         % (N // hop + 1, T))
    if unvoiced_period is None:
        unv = default_unvoiced_period(sampling_rate)
    elif isinstance(unvoiced_period, bool) or not isinstance(unvoiced_period, numbers.Integral):
        raise ValueError("unvoiced_period must be an integer number of samples or None, got %r" % (unvoiced_period,))
    else:
        unv = int(unvoiced_period)
    if not MIN_PERIOD <= unv <= MAX_PERIOD:
        raise NotImplementedError("%s holds an unvoiced_period of %d .. %d samples, got %d" % (who, MIN_PERIOD, MAX_PERIOD, unv))
    if isinstance(pace, numbers.Real) and not isinstance(pace, bool):
        paces = [float(pace)] * B
    else:
        try:
            paces = [float(p) for p in pace]
        except TypeError:
            raise ValueError("pace must be a number or a sequence of %d numbers, got %r" % (B, pace))
        if len(paces) != B:
            raise ValueError("pace must be a number or a sequence of %d numbers, got %d" % (B, len(paces)))
    for p in paces:
        if not MIN_PACE <= p <= MAX_PACE:                                   # (NaN fails both)
            raise ValueError("pace must lie in [%g, %g], got %r" % (MIN_PACE, MAX_PACE, p))
    N_out = out_samples(N, min(paces))
    if N > MAX_SAMPLES or N_out > MAX_SAMPLES:
        raise NotImplementedError("%s holds at most %d samples an utterance (MAX_SAMPLES = 2^22) before and after, got N = %d and N_out = %d"
                                  % (who, MAX_SAMPLES, N, N_out))
    if torch.is_tensor(pitch_ratio):
        r = pitch_ratio.detach()
        if r.dtype != torch.float32 or r.dim() > 2 or (r.dim() == 2 and single and r.shape[0] != 1):
            raise ValueError("pitch_ratio must be a number or a float32 [B] or [B, T] tensor, got %s %s" % (tuple(r.shape), r.dtype))
        if single and r.dim() == 1 and r.shape[0] == T:
            r = r[None]                                                     # the [T] of an [N]
        if r.dim() == 0:
            r = r.reshape(1, 1).expand(B, T)
        elif r.dim() == 1:
            if r.shape[0] != B:
                raise ValueError("pitch_ratio [B] must hold %d entries, got %d" % (B, r.shape[0]))
            r = r[:, None].expand(B, T)
        elif tuple(r.shape) != (B, T):
            raise ValueError("pitch_ratio [B, T] must have f0's shape %s, got %s" % ((B, T), tuple(r.shape)))
    elif isinstance(pitch_ratio, numbers.Real) and not isinstance(pitch_ratio, bool) and math.isfinite(pitch_ratio):
        r = float(pitch_ratio)
    else:
        raise ValueError("pitch_ratio must be a finite number or a float32 [B] or [B, T] tensor, got %r" % (pitch_ratio,))
    return a2, single, f2, r, paces, N_out, sr256, hop, unv


_HANN = {}                 # device -> the window table on it: made once, so a warm call copies one small vector of paces only


def _hann(device):
    key = str(device)
    if key not in _HANN:
        _HANN[key] = torch.from_numpy(hann_table().astype(np.float32)).to(device)
    return _HANN[key]


def _marks(a2, n32, f2, r, paces, N_out, sr256, hop, unv):
    B, N = a2.shape
    T = f2.shape[1]
    dev = a2.device
    L.require_cuda(f2)
    if not torch.is_tensor(r):
        r = torch.full((1, 1), r, dtype=torch.float32, device=dev).expand(B, T)
    L.require_cuda(r)
    KA, KS = -(-N // MIN_PERIOD), -(-N_out // (MIN_PERIOD // 2))
    if min(paces) == max(paces):                                            # one pace: a fill, nothing is copied from the host
        pq = torch.full((B,), pace_q(paces[0]), dtype=torch.int32, device=dev)
    else:
        pq = torch.tensor([pace_q(p) for p in paces], dtype=torch.int32, device=dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    m = Marks(i32(B, KA), i32(B), i32(B, KS), i32(B, KS), i32(B, KS), i32(B), i32(B))
    L.check(L.lib().ft_psola_marks(L.ptr(f2), *f2.stride(), L.ptr(r), *r.stride(), L.ptr(n32), L.ptr(pq), L.ptr(m.analysis),
                                   L.ptr(m.n_analysis), L.ptr(m.synthesis), L.ptr(m.source), L.ptr(m.half), L.ptr(m.n_synthesis),
                                   L.ptr(m.n_out), B, N, N_out, T, hop, KA, KS, sr256, unv, L.stream()), "ft_psola_marks")
    return m


# ---- the public calls ---------------------------------------------------------------------------------------------------------------

def marks(audio, n_samples, f0, sampling_rate=22050, hop_length=256, pitch_ratio=1.0, pace=1.0, unvoiced_period=None):
    """Where modify() cuts and where it lays down, the same arguments -> Marks(analysis [B, ceil(N / 16)], n_analysis [B],
    synthesis, source, half [B, ceil(N_out / 8)], n_synthesis [B], n_out [B]), int32 on the device (no leading B for [N]):
    positions in 1/256 sample; grain j is centred on (synthesis[j] + 128) >> 8 of the output, reads around
    (analysis[source[j]] + 128) >> 8 of the input and is half[j] samples wide to either side.  Entries behind an utterance's
    counts are not written.  One entry call (one launch: a wave per utterance)."""
    a2, single, f2, r, paces, N_out, sr256, hop, unv = _args("marks", audio, n_samples, f0, sampling_rate, hop_length, pitch_ratio,
                                                             pace, unvoiced_period)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    m = _marks(a2, n32, f2, r, paces, N_out, sr256, hop, unv)
    return Marks(*[x[0] for x in m]) if single else m


def modify(audio, n_samples, f0, sampling_rate=22050, hop_length=256, pitch_ratio=1.0, pace=1.0, unvoiced_period=None):
    """Change the pitch and the pace of a zero-padded batch: audio [N] or [B, N] fp32 on the device (any strides), n_samples a
    host sequence or an int32 tensor on the device (clamped to 1 ..= N; nothing behind an utterance's end is read), f0
    [B, T] Hz with 0 = unvoiced as pitch.f0 / pitch.f0_track return it at this hop_length (frame t centred on sample
    t * hop_length, T >= N // hop_length + 1, further frames ignored; NaN, inf and values <= 0 count as unvoiced)
    -> (out [B, N_out] fp32 with zeros behind each utterance, n_out int32 [B] on the device = max(1, (n << 16) // pace_q)).
    pitch_ratio: the factor on F0, a number, a [B] or a [B, T] fp32 tensor on the device (pitch_ratio() makes one), clamped to
    [0.625, 2]; unvoiced frames are never shifted, their grains are unvoiced_period samples apart (None: 5 ms).  pace: a
    number or B numbers in [0.25, 4], above 1 is faster (as align.scale_durations); N_out is out_samples(N, the smallest
    pace).  With pitch_ratio = 1 and pace = 1 the output is the input to within 1e-6 for |x| <= 1.  Two entry calls
    (ft_psola_marks, ft_psola_synth: a launch each), nothing on the host between them.
    NotImplementedError for N or N_out above 2^22 samples, more than 65,535 utterances, an unvoiced_period outside 16 .. 1024."""
    a2, single, f2, r, paces, N_out, sr256, hop, unv = _args("modify", audio, n_samples, f0, sampling_rate, hop_length, pitch_ratio,
                                                             pace, unvoiced_period)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    m = _marks(a2, n32, f2, r, paces, N_out, sr256, hop, unv)
    B, N = a2.shape
    out = torch.empty(B, N_out, dtype=torch.float32, device=a2.device)
    L.check(L.lib().ft_psola_synth(L.ptr(a2), *a2.stride(), L.ptr(n32), L.ptr(m.analysis), L.ptr(m.synthesis), L.ptr(m.source),
                                   L.ptr(m.half), L.ptr(m.n_synthesis), L.ptr(m.n_out), L.ptr(_hann(a2.device)), L.ptr(out), B, N,
                                   N_out, m.analysis.shape[1], m.synthesis.shape[1], L.stream()), "ft_psola_synth")
    return (out[0], m.n_out[0]) if single else (out, m.n_out)


# ---- a pace that varies within the utterance: the marks walk a time map ---------------------------------------------------------------
#
#     mcd, path, plen = metrics.mel_cepstral_distortion(mel_syn, lens, mel_rec, rec_lens, return_path=True)
#     tmap = prosody.time_map_from_path(path, plen, hop, n_frames=mel_rec.shape[2])          # recording frame -> synthesized position
#     ratio = prosody.transfer_ratio(f0_syn, f0_rec, tmap, hop, register="source")           # the recording's melody, this voice's register
#     out, n_out = prosody.warp(audio, n, f0_syn, tmap, rec_samples, hop_length=hop, pitch_ratio=ratio, ratio_axis="output")
#
# A time map is int32 [B, TM]: entry u is the input position, in 1 / 256 sample, that output sample u * out_hop_length plays; between
# entries the walk interpolates, it never goes back (a decreasing stretch holds the input still) and never leaves the utterance.

MAX_PATH = 4096            # FT_PSOLA_MAX_PATH: cells of a warping path
MAX_SMOOTH = 32            # FT_PSOLA_MAX_SMOOTH
_AXES = {"input": 0, "output": 1}


def time_map_from_path(path, path_len, hop_length, n_frames, smooth=4):
    """A warping path -> the time map that plays the source along it: path [B, P, 2] int32 on the device, cells (source frame,
    reference frame) in ascending order, and path_len [B] int32, as metrics.dtw(source, reference) or
    metrics.mel_cepstral_distortion(mel_source, lens, mel_reference, ref_lens, return_path=True) return them; both sides at
    hop_length -> tmap [B, n_frames + 1] int32 on the device, for warp(..., out_hop_length=hop_length) and an output of up to
    n_frames * hop_length - 1 samples (n_frames: the reference's frames or more).  Reference frame u plays the middle of the
    source frames the path matched to it, 128 hop_length (lowest + highest), averaged over the 2 smooth + 1 frames around u
    (indices held inside the path's reference frames; integers, truncating), so a staircase path does not become freezes and
    jumps; entries behind the path's last reference frame repeat the end.  One entry call (ft_psola_time_map: one launch), no
    synchronisation.  NotImplementedError for more than 4096 cells."""
    if not torch.is_tensor(path) or path.dtype != torch.int32 or path.dim() != 3 or path.shape[2] != 2 or min(path.shape) < 1:
        raise ValueError("path must be an int32 [B, P, 2] tensor as metrics.dtw returns it, got %s"
                         % ((tuple(path.shape), path.dtype) if torch.is_tensor(path) else type(path).__name__,))
    B, P = path.shape[0], path.shape[1]
    if not torch.is_tensor(path_len) or path_len.dtype != torch.int32 or tuple(path_len.shape) != (B,):
        raise ValueError("path_len must be an int32 [%d] tensor as metrics.dtw returns it, got %s"
                         % (B, (tuple(path_len.shape), path_len.dtype) if torch.is_tensor(path_len) else type(path_len).__name__))
    hop = _int_arg(hop_length, "hop_length", 1)
    TM = _int_arg(n_frames, "n_frames", 1) + 1
    w = _int_arg(smooth, "smooth", 0)
    if w > MAX_SMOOTH:
        raise ValueError("smooth must lie in 0 ..= %d frames, got %d" % (MAX_SMOOTH, w))
    if hop > MAX_SAMPLES:
        raise ValueError("hop_length must not exceed MAX_SAMPLES = %d, got %d" % (MAX_SAMPLES, hop))
    if B > MAX_BATCH:
        raise NotImplementedError("time_map_from_path holds at most %d utterances a call, got %d" % (MAX_BATCH, B))
    if P > MAX_PATH:
        raise NotImplementedError("time_map_from_path holds at most %d cells a path (MAX_PATH), got %d" % (MAX_PATH, P))
    L.require_cuda(path, path_len)
    cells, plen = path.detach().contiguous(), path_len.detach().contiguous()
    tmap = torch.empty(B, TM, dtype=torch.int32, device=path.device)
    L.check(L.lib().ft_psola_time_map(L.ptr(cells), L.ptr(plen), L.ptr(tmap), B, P, TM, hop, w, L.stream()), "ft_psola_time_map")
    return tmap


def time_map_from_durations(src_durations, tgt_durations, in_lens, hop_length, n_frames=None):
    """Token durations before and after -> the time map that gives every token its new length (per-token emphasis: "slow down
    this one word"): src_durations and tgt_durations [B, L] integer frames per token (align.monotonic_alignment's durations and
    an edited copy; negative counts as 0), in_lens [B] tokens (a sequence or a tensor; None: L; tokens behind it count as 0
    frames) -> (tmap [B, n_frames + 2] int32, n_out_frames [B] int32: the target's frames), on the durations' device.
    With S_l, E_l the first frame of token l before and after (running sums), d_l, e_l its frames before and after, Qh = 256
    hop_length:   tmap[u] = Qh S_l + (Qh d_l (u - E_l)) // e_l   for E_l <= u < E_{l+1}   (a token with e_l = 0 is skipped: no u
    lies in it; a boundary is hit exactly, tmap[E_l] = Qh S_l),   tmap[u] = Qh S_total   for u at or behind the target's total;
    int64, held to 0 ..= 2^31 - 1.  Plain integer torch (cumsum, searchsorted, gather).  n_frames: the width is given by the
    caller and nothing synchronises; None: the largest target total, read from the device (one synchronisation)."""
    for d, name in ((src_durations, "src_durations"), (tgt_durations, "tgt_durations")):
        if not torch.is_tensor(d) or d.dim() != 2 or d.dtype.is_floating_point or d.dtype == torch.bool or min(d.shape) < 1:
            raise ValueError("%s must be an integer [B, L] tensor, got %s" % (name, (tuple(d.shape), d.dtype) if torch.is_tensor(d) else type(d).__name__))
    if src_durations.shape != tgt_durations.shape:
        raise ValueError("src_durations and tgt_durations must have one shape, got %s and %s" % (tuple(src_durations.shape), tuple(tgt_durations.shape)))
    hop = _int_arg(hop_length, "hop_length", 1)
    B, Lt = src_durations.shape
    dev = src_durations.device
    d = src_durations.detach().to(torch.int64).clamp(min=0)
    e = tgt_durations.detach().to(dev, torch.int64).clamp(min=0)
    if in_lens is not None:
        if torch.is_tensor(in_lens):
            ln = in_lens.detach().to(dev).reshape(-1)
        else:
            ln = torch.tensor([int(v) for v in in_lens], device=dev)
        if ln.shape[0] != B:
            raise ValueError("in_lens must hold %d entries, got %d" % (B, ln.shape[0]))
        keep = torch.arange(Lt, device=dev)[None, :] < ln[:, None]
        d, e = d * keep, e * keep
    src_end, tgt_end = d.cumsum(1), e.cumsum(1)
    total = tgt_end[:, -1]
    U = (int(total.max()) if n_frames is None else _int_arg(n_frames, "n_frames", 1)) + 2
    u = torch.arange(U, device=dev, dtype=torch.int64)[None, :].expand(B, U).contiguous()
    l = torch.searchsorted(tgt_end, u, right=True)                           # the tokens that end at or before u
    behind = l >= Lt
    lc = l.clamp(max=Lt - 1)
    S, E = (src_end - d).gather(1, lc), (tgt_end - e).gather(1, lc)
    dl, el = d.gather(1, lc), e.gather(1, lc).clamp(min=1)
    qh = Q * hop
    inside = qh * S + torch.div(qh * dl * (u - E), el, rounding_mode="floor")
    tmap = torch.where(behind, (qh * src_end[:, -1])[:, None].expand(B, U), inside).clamp(0, 2 ** 31 - 1).to(torch.int32)
    return tmap, total.to(torch.int32)


def transfer_ratio(f0_src, f0_ref, time_map, hop_length, src_lens=None, ref_lens=None, register="reference"):
    """The per-frame factor that gives the source the reference's melody, on the OUTPUT's frames (warp(..., ratio_axis="output")):
    f0_src [B, T_src] and f0_ref [B, T_ref] Hz with 0 = unvoiced (or [T_src], [T_ref]), time_map [B, TM >= T_ref] int32 at
    hop_length on both sides, src_lens / ref_lens their frames (None: all; frames behind count as unvoiced) -> [B, T_ref] fp32.
    Output frame u plays source frame t = min(T_src - 1, ((time_map[u] >> 8) + hop_length // 2) // hop_length); where f0_ref[u] and
    f0_src[t] are both voiced the factor is f0_ref[u] c / f0_src[t], elsewhere 1.  register="reference": c = 1, the output takes
    the reference's pitch itself.  register="source": c moves the reference's contour onto the source's voiced mean of log f0
    (the mean pitch_ratio uses), the melody's shape in the speaker's own register.  float64 torch on the tensors' device,
    rounded once; no synchronisation.  warp clamps the factor to [0.625, 2]."""
    for f, name in ((f0_src, "f0_src"), (f0_ref, "f0_ref")):
        if not torch.is_tensor(f) or f.dim() not in (1, 2) or not f.dtype.is_floating_point or min(f.shape) < 1:
            raise ValueError("%s must be a floating [T] or [B, T] tensor, got %s" % (name, (tuple(f.shape) if torch.is_tensor(f) else type(f).__name__),))
    if f0_src.dim() != f0_ref.dim():
        raise ValueError("f0_src and f0_ref must both be [T] or both [B, T], got %s and %s" % (tuple(f0_src.shape), tuple(f0_ref.shape)))
    single = f0_src.dim() == 1
    fs, fr = (f0_src[None], f0_ref[None]) if single else (f0_src, f0_ref)
    B, Ts = fs.shape
    Tr = fr.shape[1]
    if fr.shape[0] != B:
        raise ValueError("f0_src holds %d utterances and f0_ref %d" % (B, fr.shape[0]))
    if not torch.is_tensor(time_map) or time_map.dtype != torch.int32 or time_map.dim() != fs.dim() - (1 if single else 0):
        raise ValueError("time_map must be an int32 %s tensor, got %s" % ("[TM]" if single else "[B, TM]",
                         (tuple(time_map.shape), time_map.dtype) if torch.is_tensor(time_map) else type(time_map).__name__))
    tm = time_map[None] if single else time_map
    if tm.shape[0] != B or tm.shape[1] < Tr:
        raise ValueError("time_map must hold %d rows of at least T_ref = %d entries, got %s" % (B, Tr, tuple(tm.shape)))
    hop = _int_arg(hop_length, "hop_length", 1)
    if register not in ("reference", "source"):
        raise ValueError("register must be 'reference' or 'source', got %r" % (register,))
    dev = fs.device

    def voiced_of(f, lens, name):
        v = (f > 0) & torch.isfinite(f)
        if lens is None:
            return v
        if torch.is_tensor(lens):
            ln = lens.to(dev).reshape(-1)
        else:
            ln = torch.tensor([int(x) for x in lens], device=dev)
        if ln.shape[0] != B:
            raise ValueError("%s must hold %d entries, got %d" % (name, B, ln.shape[0]))
        return v & (torch.arange(f.shape[1], device=dev)[None, :] < ln[:, None])

    vs, vr = voiced_of(fs, src_lens, "src_lens"), voiced_of(fr, ref_lens, "ref_lens")
    t = (((tm[:, :Tr].to(dev, torch.int64) >> 8) + hop // 2) // hop).clamp(0, Ts - 1)
    one = torch.ones((), dtype=torch.float64, device=dev)
    both = vr & vs.gather(1, t)
    src_at = torch.where(both, fs.double().gather(1, t), one)
    ref = torch.where(both, fr.double(), one)
    if register == "source":
        mean = lambda f, v: (torch.log2(torch.where(v, f.double(), one)).sum(1) / v.sum(1).double())[:, None]
        c = torch.exp2(mean(fs, vs) - mean(fr, vr))                          # NaN where either has no voiced frame: no frame reads it
        ref = torch.where(both, ref * c, one)
    ratio = (ref / src_at).to(torch.float32)
    return ratio[0] if single else ratio


def _warp_args(who, audio, n_samples, f0, time_map, n_out, sampling_rate, hop_length, out_hop_length, pitch_ratio, ratio_axis,
               unvoiced_period, max_out):
    """every check that needs no device -> what _warp_marks takes"""
    a2, single, f2, _, _, _, sr256, hop, unv = _args(who, audio, n_samples, f0, sampling_rate, hop_length, 1.0, 1.0, unvoiced_period)
    B, N = a2.shape
    T = f2.shape[1]
    hop_out = hop if out_hop_length is None else _int_arg(out_hop_length, "out_hop_length", 1)
    if hop_out > MAX_SAMPLES:
        raise ValueError("out_hop_length must not exceed MAX_SAMPLES = %d, got %d" % (MAX_SAMPLES, hop_out))
    if ratio_axis not in _AXES:
        raise ValueError("ratio_axis must be 'input' or 'output', got %r" % (ratio_axis,))
    axis = _AXES[ratio_axis]
    if not torch.is_tensor(time_map) or time_map.dtype != torch.int32 or time_map.dim() != (1 if single else 2) or \
            (time_map[None] if single else time_map).shape[0] != B:
        raise ValueError("time_map must be an int32 %s tensor of input positions in 1/256 sample, got %s"
                         % ("[TM]" if single else "[%d, TM]" % B, (tuple(time_map.shape), time_map.dtype) if torch.is_tensor(time_map)
                            else type(time_map).__name__))
    tm = (time_map[None] if single else time_map).detach()
    if max_out is not None:
        max_out = _int_arg(max_out, "max_out", 1)
    if torch.is_tensor(n_out) and n_out.is_cuda:
        if n_out.dtype != torch.int32 or n_out.numel() != B or n_out.dim() > 1 or (n_out.dim() == 0 and not single):
            raise ValueError("n_out on the device must be an int32 [%d] tensor, got %s %s" % (B, tuple(n_out.shape), n_out.dtype))
        if max_out is None:
            raise ValueError("max_out (the output's width) must be given when n_out is a tensor on the device: reading it would synchronise")
        no32, N_out = n_out.detach().reshape(B).contiguous(), max_out
    else:
        try:
            host = [n_out] if isinstance(n_out, numbers.Integral) and not isinstance(n_out, bool) else \
                (n_out.reshape(-1).tolist() if torch.is_tensor(n_out) else list(n_out))
        except TypeError:
            raise ValueError("n_out must be a sequence of %d integers or an int32 tensor on the device, got %r" % (B, n_out))
        if len(host) != B or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1 for v in host):
            raise ValueError("n_out must hold %d integers >= 1 (the samples of every output), got %r" % (B, host))
        no32, N_out = [int(v) for v in host], max(int(v) for v in host)
        if max_out is not None:
            if max_out < N_out:
                raise ValueError("max_out = %d is below the largest n_out = %d" % (max_out, N_out))
            N_out = max_out
    if N_out > MAX_SAMPLES:
        raise NotImplementedError("%s holds at most %d samples an utterance (MAX_SAMPLES = 2^22) before and after, got N = %d and N_out = %d"
                                  % (who, MAX_SAMPLES, N, N_out))
    if tm.shape[1] < N_out // hop_out + 2:
        raise ValueError("time_map must hold at least N_out // out_hop_length + 2 = %d entries (entry u is output sample u * out_hop_length), got %d"
                         % (N_out // hop_out + 2, tm.shape[1]))
    RT = T if axis == 0 else N_out // hop_out + 1
    if torch.is_tensor(pitch_ratio):
        r = pitch_ratio.detach()
        if r.dtype != torch.float32 or r.dim() > 2 or (r.dim() == 2 and single and r.shape[0] != 1):
            raise ValueError("pitch_ratio must be a number or a float32 [B] or [B, T] tensor, got %s %s" % (tuple(r.shape), r.dtype))
        if single and r.dim() == 1 and r.shape[0] != 1:
            r = r[None]                                                     # the [T] of an [N]
        if r.dim() == 0:
            r = r.reshape(1, 1).expand(B, RT)
        elif r.dim() == 1:
            if r.shape[0] != B:
                raise ValueError("pitch_ratio [B] must hold %d entries, got %d" % (B, r.shape[0]))
            r = r[:, None].expand(B, RT)
        elif r.shape[0] != B or (r.shape[1] != T if axis == 0 else r.shape[1] < RT):
            raise ValueError("pitch_ratio [B, T] must have %s, got %s"
                             % ("f0's shape %s (ratio_axis='input')" % ((B, T),) if axis == 0 else
                                "%d rows of at least N_out // out_hop_length + 1 = %d output frames (ratio_axis='output')" % (B, RT), tuple(r.shape)))
    elif isinstance(pitch_ratio, numbers.Real) and not isinstance(pitch_ratio, bool) and math.isfinite(pitch_ratio):
        r = float(pitch_ratio)
    else:
        raise ValueError("pitch_ratio must be a finite number or a float32 [B] or [B, T] tensor, got %r" % (pitch_ratio,))
    return a2, single, f2, r, tm, no32, N_out, sr256, hop, hop_out, axis, unv


def _warp_marks(a2, n32, f2, r, tm, no32, N_out, sr256, hop, hop_out, axis, unv):
    B, N = a2.shape
    T = f2.shape[1]
    dev = a2.device
    L.require_cuda(f2, tm)
    if not torch.is_tensor(r):
        r = torch.full((1, 1), r, dtype=torch.float32, device=dev).expand(B, T if axis == 0 else N_out // hop_out + 1)
    L.require_cuda(r)
    if not torch.is_tensor(no32):
        no32 = torch.tensor(no32, dtype=torch.int32, device=dev)
    tm = tm.contiguous()
    KA, KS = -(-N // MIN_PERIOD), -(-N_out // (MIN_PERIOD // 2))
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    m = Marks(i32(B, KA), i32(B), i32(B, KS), i32(B, KS), i32(B, KS), i32(B), i32(B))
    L.check(L.lib().ft_psola_marks_warp(L.ptr(f2), *f2.stride(), L.ptr(r), *r.stride(), L.ptr(n32), L.ptr(no32), L.ptr(tm),
                                        L.ptr(m.analysis), L.ptr(m.n_analysis), L.ptr(m.synthesis), L.ptr(m.source), L.ptr(m.half),
                                        L.ptr(m.n_synthesis), L.ptr(m.n_out), B, N, N_out, T, r.shape[1], tm.shape[1], hop, hop_out, axis,
                                        KA, KS, sr256, unv, L.stream()), "ft_psola_marks_warp")
    return m


def warp_marks(audio, n_samples, f0, time_map, n_out, sampling_rate=22050, hop_length=256, out_hop_length=None, pitch_ratio=1.0,
               ratio_axis="input", unvoiced_period=None, max_out=None):
    """Where warp() cuts and where it lays down, the same arguments -> Marks as marks() returns them.  One entry call
    (ft_psola_marks_warp: one launch, a wave per utterance)."""
    a2, single, f2, r, tm, no32, N_out, sr256, hop, hop_out, axis, unv = _warp_args(
        "warp_marks", audio, n_samples, f0, time_map, n_out, sampling_rate, hop_length, out_hop_length, pitch_ratio, ratio_axis,
        unvoiced_period, max_out)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    m = _warp_marks(a2, n32, f2, r, tm, no32, N_out, sr256, hop, hop_out, axis, unv)
    return Marks(*[x[0] for x in m]) if single else m


def warp(audio, n_samples, f0, time_map, n_out, sampling_rate=22050, hop_length=256, out_hop_length=None, pitch_ratio=1.0,
         ratio_axis="input", unvoiced_period=None, max_out=None):
    """modify() with a pace that varies within the utterance: audio, n_samples, f0, sampling_rate, hop_length and unvoiced_period
    as modify takes them; time_map [B, TM] int32 on the device (or [TM] for [N]): entry u is the input position, in 1/256
    sample, that output sample u * out_hop_length plays (None: hop_length), TM >= N_out // out_hop_length + 2 -- from
    time_map_from_path, time_map_from_durations or your own; between entries the position is interpolated, it never goes back (a
    decreasing stretch of the map holds the input still) and is held inside the utterance, whatever the map holds.  n_out: the
    samples of every output, a host sequence of B integers >= 1 or an int32 [B] tensor on the device (clamped to 1 ..= N_out);
    N_out = max(n_out), or max_out, which must be given when n_out is on the device.
    -> (out [B, N_out] fp32 with zeros behind each utterance, n_out int32 [B] on the device).
    pitch_ratio: a number, a [B] tensor, or per frame -- ratio_axis="input": [B, T] on f0's frames as in modify;
    ratio_axis="output": [B, RT >= N_out // out_hop_length + 1] on the OUTPUT's frames (frame u centred on output sample
    u * out_hop_length), which is where a target contour lives (transfer_ratio makes one); clamped to [0.625, 2], unvoiced input
    frames are never shifted.  With time_map[u] = u * hop_length * 256 * pace and n_out = out_samples(n, pace) the result is
    modify's at pace 1, 2 and 0.5, bit for bit.  Two entry calls (ft_psola_marks_warp, ft_psola_synth: a launch each), nothing on
    the host between them.  NotImplementedError for N or N_out above 2^22 samples, more than 65,535 utterances, an
    unvoiced_period outside 16 .. 1024."""
    a2, single, f2, r, tm, no32, N_out, sr256, hop, hop_out, axis, unv = _warp_args(
        "warp", audio, n_samples, f0, time_map, n_out, sampling_rate, hop_length, out_hop_length, pitch_ratio, ratio_axis,
        unvoiced_period, max_out)
    n32, _ = _lengths(n_samples, a2)
    L.require_cuda(a2)
    m = _warp_marks(a2, n32, f2, r, tm, no32, N_out, sr256, hop, hop_out, axis, unv)
    B, N = a2.shape
    out = torch.empty(B, N_out, dtype=torch.float32, device=a2.device)
    L.check(L.lib().ft_psola_synth(L.ptr(a2), *a2.stride(), L.ptr(n32), L.ptr(m.analysis), L.ptr(m.synthesis), L.ptr(m.source),
                                   L.ptr(m.half), L.ptr(m.n_synthesis), L.ptr(m.n_out), L.ptr(_hann(a2.device)), L.ptr(out), B, N,
                                   N_out, m.analysis.shape[1], m.synthesis.shape[1], L.stream()), "ft_psola_synth")
    return (out[0], m.n_out[0]) if single else (out, m.n_out)


def pitch_ratio(f0, lens=None, shift_semitones=0.0, range_scale=1.0):
    """The per-frame factor that moves and scales an utterance's intonation: f0 [B, T] (or [T]) Hz with 0 = unvoiced, lens its
    frames (None: T) -> [B, T] fp32.  On a voiced frame the target is log f0' = mean + range_scale (log f0 - mean) + shift,
    mean the utterance's voiced-frame mean of log f0 (the one pitch.f0_statistics reports), and the result f0' / f0; 1 on an
    unvoiced frame.  range_scale = 0 is a monotone reading, 2 twice the range.  Plain float64 torch on the tensor's device,
    rounded once; no synchronisation."""
    if not torch.is_tensor(f0) or f0.dim() not in (1, 2) or not f0.dtype.is_floating_point or min(f0.shape) < 1:
        raise ValueError("f0 must be a floating [T] or [B, T] tensor, got %s" % ((tuple(f0.shape) if torch.is_tensor(f0) else type(f0).__name__),))
    for v, name in ((shift_semitones, "shift_semitones"), (range_scale, "range_scale")):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
            raise ValueError("%s must be a finite number, got %r" % (name, v))
    f = f0[None] if f0.dim() == 1 else f0
    B, T = f.shape
    voiced = (f > 0) & torch.isfinite(f)
    if lens is not None:
        if torch.is_tensor(lens):
            ln = lens.to(f.device).reshape(B)
        else:
            if len(lens) != B:
                raise ValueError("lens must hold %d entries, got %d" % (B, len(lens)))
            ln = torch.tensor([int(v) for v in lens], device=f.device)
        voiced = voiced & (torch.arange(T, device=f.device)[None, :] < ln[:, None])
    one = torch.ones((), dtype=torch.float64, device=f.device)
    lf = torch.log2(torch.where(voiced, f.double(), one))
    mean = (lf.sum(1) / voiced.sum(1).double())[:, None]                     # NaN where nothing is voiced: no frame reads it
    target = mean + float(range_scale) * (lf - mean) + float(shift_semitones) / 12.0
    ratio = torch.where(voiced, torch.exp2(target - lf), one).to(torch.float32)
    return ratio[0] if f0.dim() == 1 else ratio
