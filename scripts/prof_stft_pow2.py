"""The power-of-two STFT kernels on a 44.1 kHz batch (32 x 10 s, n_fft 2048, hop 512): ms per batch of the ragged mel in one
launch against the per-utterance ft_stft_mel loop the data path ran before, STFT.transform, STFT.inverse and one Griffin-Lim
iteration (transform + inverse: the loop body of griffin_lim after its host draw of the starting angles).  A stand-alone
workload for rocprofv3 passes too."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import audio_processing
from flowtron_amd import _lib as L

B, SR, N, NFFT, HOP = 32, 44100, 441000, 2048, 512


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    tst = audio_processing.TacotronSTFT(NFFT, HOP, NFFT, 80, SR, 0.0, 8000.0).cuda()
    st = tst.stft_fn
    g = torch.Generator().manual_seed(0)
    y = ((torch.rand(B, N, generator=g) * 2 - 1) * 0.9).cuda()
    lens = torch.randint(N // 2, N + 1, (B,), generator=g)
    lens[0] = N
    for i, n in enumerate(lens.tolist()):
        y[i, n:] = 0
    ns = lens.to(torch.int32).cuda()
    T = N // HOP + 1
    frames = int((lens // HOP + 1).sum())

    ragged = timed(lambda: tst.mel_spectrogram_ragged(y, ns, T))
    mel = torch.zeros(B, 80, T, device="cuda")

    def loop():                                    # the data path before: one ft_stft_mel launch per utterance
        for i, n in enumerate(lens.tolist()):
            L.check(L.lib().ft_stft_mel(L.ptr(y[i]), L.ptr(st.fft_window), L.ptr(tst.mel_basis), L.ptr(mel[i]), 1, n, NFFT, HOP,
                                        80, L.stream()), "ft_stft_mel")
    per_utt = timed(loop)
    mag, ph = st.transform(y)
    transform = timed(lambda: st.transform(y))
    inverse = timed(lambda: st.inverse(mag, ph))
    sig = st.inverse(mag, ph).squeeze(1)

    def gl_iteration():                            # the loop body of griffin_lim: new phase from the signal, then the signal
        _, angles = st.transform(sig)
        st.inverse(mag, angles)
    gl = timed(gl_iteration)
    print("batch %d x %.0f s at %d Hz, n_fft %d, hop %d: %d frames" % (B, N / SR, SR, NFFT, HOP, frames))
    print("ragged mel, one launch      : %.3f ms per batch" % ragged)
    print("ft_stft_mel per utterance   : %.3f ms per batch (%d launches)" % (per_utt, B))
    print("STFT.transform (mag + phase): %.3f ms per batch" % transform)
    print("STFT.inverse                : %.3f ms per batch" % inverse)
    print("one Griffin-Lim iteration   : %.3f ms per batch" % gl)


if __name__ == "__main__":
    main()
