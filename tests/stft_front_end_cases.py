"""The inputs of the front end's float64 tests, shared by test_stft_ref64_cpu.py (which checks, without a GPU, that the bounds
of tests/stft_ref64.py mean something on exactly these inputs) and test_gpu_stft_front_end_f64.py (which holds the kernels to
them).  Audio is oracle.synth.make_audio; nothing here touches a device."""
import numpy as np
import torch

from flowtron_amd.audio import slaney_mel_filterbank
from stft_ref64 import csr_dense64, handmade_csr

# ---- A: (hop, win, B, N) of the r8 transform (n_fft 1024).  Odd hops 1 and 255 (a frame's float2 reads 4-byte aligned only),
# win < n_fft, the shortest signal 513, and frame counts 15 | 16 | 16 | 17 (workgroup edge) and 4 | 5 (wave edge).
A_GRID = [
    (256, 1024, 3, 256 * 40 + 255),
    (200, 800, 2, 8000),
    (128, 1024, 1, 513),
    (1, 1024, 1, 600),
    (255, 257, 2, 4079),
    (256, 256, 1, 4095),
    (64, 1000, 1, 3000),
    (256, 1024, 1, 3839),
    (256, 1024, 1, 3840),
    (256, 1024, 1, 4095),
    (256, 1024, 1, 4096),
    (256, 1024, 1, 768),
    (256, 1024, 1, 1024),
]
A_IDS = ["h%d_w%d_B%d_N%d" % g for g in A_GRID]

# ---- B: Slaney filterbanks (sr, n_mel, fmin, fmax) x (hop, win) at n_fft 1024
B_BANKS = [
    (22050, 80, 0.0, 8000.0),
    (22050, 128, 0.0, None),
    (16000, 80, 90.0, 7600.0),
    (22050, 1, 0.0, None),
    (22050, 64, 0.0, 8000.0),
    (22050, 65, 0.0, 8000.0),
]
B_HOPS = [(256, 1024), (200, 800), (255, 1024)]
B_SHAPE = (2, 5221)                                      # 21 | 27 | 21 frames: a full workgroup and a part of one
B_CASES = [bank + hw for bank in B_BANKS for hw in B_HOPS]
B_IDS = ["sr%d_m%d_h%d_w%d" % (c[0], c[1], c[4], c[5]) for c in B_CASES]
SILENCE_N = 6000

# ---- C: the hand-made filterbanks (kind, n_fft, hop); 19 or 20 frames: not a multiple of 16
C_CASES = [(kind, n_fft, hop) for kind in ("WIDE", "NARROW") for n_fft in (1024, 512) for hop in (256, 255)]
C_IDS = ["%s_n%d_h%d" % c for c in C_CASES]
C_SHAPE = (2, 4900)

# ---- D: lengths of the ragged batch (the last is the padded width), and the short utterance
D_LENS = [513, 3 * 1024 + 17, 256 * 16 - 1, 256 * 16, 5000]
D_SHORT = 300

# ---- E: ft_stft_mel's own settings (sr, n_fft, hop, win, n_mel, B, N)
E_CASES = [
    (22050, 1024, 256, 1024, 129, 2, 2500),              # 10 frames: one full workgroup of 8 and a part
    (22050, 1024, 256, 1024, 160, 1, 513),               # N = n_fft / 2 + 1
    (16000, 128, 32, 128, 40, 2, 1000),                  # 32 frames
    (16000, 64, 16, 64, 20, 1, 33),                      # N = n_fft / 2 + 1 at the smallest size: 3 frames
    (16000, 64, 16, 64, 20, 3, 1111),                    # 70 frames
    (16000, 512, 384, 256, 80, 2, 4000),                 # hop above win_length
    (44100, 4096, 1024, 4096, 160, 1, 9000),             # 9 frames
]
E_IDS = ["n%d_h%d_w%d_m%d_N%d" % (c[1], c[2], c[3], c[4], c[6]) for c in E_CASES]


def audio(B, N, seed):
    from oracle import synth
    return torch.stack([synth.make_audio(N, seed=seed + i) for i in range(B)]).numpy()


def audio_a(hop, win, B, N):
    return audio(B, N, seed=1000 + hop + win + N)


def audio_b(hop):
    return audio(*B_SHAPE, seed=2000 + hop)


def silence():
    """[1, SILENCE_N]: the first third at 1e-4 of full scale, the rest exactly zero."""
    y = audio(1, SILENCE_N, seed=2999)
    y[:, :SILENCE_N // 3] *= np.float32(1e-4)
    y[:, SILENCE_N // 3:] = 0.0
    return y


def silent_frames(n_fft, hop, N=SILENCE_N):
    """The frames of silence() whose n_fft samples, reflections included, are all zeros."""
    t = np.arange(N // hop + 1)
    return t * hop - n_fft // 2 >= N // 3


def audio_c(n_fft, hop):
    return audio(*C_SHAPE, seed=3000 + n_fft + hop)


def audio_d(i, n):
    return audio(1, n, seed=4000 + i)[0]


def audio_e(case):
    sr, n_fft, hop, win, n_mel, B, N = case
    return audio(B, N, seed=5000 + n_fft + hop + n_mel + N)


# ---- F (and the CPU margin test): (input name of mel_inputs(), the wrong references that apply to it).  The floor shows only
# where a band sum is below 1e-5: in the silence input, and in the empty band of a hand-made filterbank.  The one-band
# filterbank's last weight is ~0, so dropping it changes nothing.
F_B, F_C = "B_sr22050_m80_h256_w1024", "C_WIDE_n1024_h255"
MUTATION_INPUTS = [
    (F_B, ["edge_reflect", "drop_last_bin", "bin0_shift", "symmetric_hann", "frame_offset"]),
    (F_C, ["edge_reflect", "drop_last_bin", "bin0_shift", "floor_1e-6", "symmetric_hann", "frame_offset"]),
    ("B_sr22050_m1_h256_w1024", ["bin0_shift"]),
    ("B_silence", ["floor_1e-6"]),
]


def slaney(sr, n_mel, fmin, fmax, n_fft=1024):
    """The float32 filterbank TacotronSTFT builds for these settings."""
    return slaney_mel_filterbank(sr, n_fft, n_mel, fmin, fmax)


def handmade_dense(kind, n_fft):
    return csr_dense64(*handmade_csr(kind, n_fft // 2 + 1), n_fft // 2 + 1)


def mel_inputs():
    """Every (name, y, (n_fft, hop, win), fb float64) of sections B, C and E that goes through a filterbank: what the fp32
    stand-in must pass logmel_judge on."""
    for c, name in zip(B_CASES, B_IDS):
        sr, n_mel, fmin, fmax, hop, win = c
        yield "B_" + name, audio_b(hop), (1024, hop, win), slaney(sr, n_mel, fmin, fmax).astype(np.float64)
    yield "B_silence", silence(), (1024, 256, 1024), slaney(*B_BANKS[0]).astype(np.float64)
    for c, name in zip(C_CASES, C_IDS):
        kind, n_fft, hop = c
        yield "C_" + name, audio_c(n_fft, hop), (n_fft, hop, n_fft), handmade_dense(kind, n_fft)
    for i, n in enumerate(D_LENS):
        yield "D_utt%d" % i, audio_d(i, n)[None], (1024, 256, 1024), slaney(*B_BANKS[0]).astype(np.float64)
    for c, name in zip(E_CASES, E_IDS):
        sr, n_fft, hop, win, n_mel, B, N = c
        yield "E_" + name, audio_e(c), (n_fft, hop, win), slaney(sr, n_mel, 0.0, None, n_fft).astype(np.float64)
