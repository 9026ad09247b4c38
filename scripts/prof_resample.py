"""Sample-rate conversion on the device (audio_processing.resample_ragged: one ft_resample_ragged launch per batch) at B = 32
utterances of up to 10 s and mixed length, 24 000 -> 22 050 Hz and 48 000 -> 22 050 Hz: device-event time of warm calls, median of
--reps runs, as whole calls (lengths to the device, output allocation, launch) and as the launch alone; the fraction of the
HBM peak (8.0 TB/s, datasheet) that (bytes read + bytes written) / time reaches; and the mel front end
(TacotronSTFT.mel_spectrogram_ragged, 1024 / 256) on the resampled batch beside it, so the reader sees what resampling adds to a
batch's `.cuda()`.  One process; run it under a time limit (timeout -k 10 300 python scripts/prof_resample.py).
A stand-alone workload for rocprofv3 passes too (--reps 1 --warmup 1)."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import audio_processing
from flowtron_amd import audio as A

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=32)
a = ap.parse_args()
HBM_PEAK = 8.0e12
TARGET = 22050
stft = audio_processing.TacotronSTFT(1024, 256, 1024, 80, TARGET, 0.0, 8000.0).cuda()


def timed(fn):
    us = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return np.array(us)


for orig in (24000, 48000):
    rs = np.random.RandomState(orig)
    lens = [int(s * orig) for s in rs.uniform(3.0, 10.0, a.batch)]
    lens[0] = 10 * orig
    x = torch.randn(a.batch, max(lens), device="cuda").clamp_(-1, 1)
    ns = A._lengths_to_device(lens, x.device)
    n_out = [A.resample_length(n, orig, TARGET) for n in lens]
    ns_out = A._lengths_to_device(n_out, x.device)
    cases = [("whole call", lambda: audio_processing.resample_ragged(x, lens, orig, TARGET)),
             ("launch alone", lambda: A._resample_launch(x, ns, orig, TARGET, max(n_out)))]
    y = None
    for name, fn in cases:
        for _ in range(a.warmup):
            y = fn()
        torch.cuda.synchronize()
        us = timed(fn)
        nbytes = 4 * (sum(lens) + a.batch * max(n_out))          # the samples read + every output written (zeros behind too)
        print("resample_ragged %d -> %d, B=%d, %.1f .. %.1f s: %s median %.1f us (min %.1f, max %.1f, %d runs), %.1f MB, "
              "%.0f GB/s = %.1f %% of the 8.0 TB/s HBM peak" % (orig, TARGET, a.batch, min(lens) / orig, max(lens) / orig, name,
                                                               np.median(us), us.min(), us.max(), a.reps, nbytes / 1e6,
                                                               nbytes / (np.median(us) * 1e-6) / 1e9,
                                                               100 * nbytes / (np.median(us) * 1e-6) / HBM_PEAK), flush=True)
    y = y[0] if isinstance(y, tuple) else y
    for _ in range(a.warmup):
        stft.mel_spectrogram_ragged(y, ns_out)
    torch.cuda.synchronize()
    us = timed(lambda: stft.mel_spectrogram_ragged(y, ns_out))
    print("mel_spectrogram_ragged on that batch (B=%d, up to %d samples): median %.1f us (min %.1f, max %.1f, %d runs)"
          % (a.batch, y.shape[1], np.median(us), us.min(), us.max(), a.reps), flush=True)
