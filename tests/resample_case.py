"""A mixed-rate data set on disk for the resampling tests: int16 wavs of mixed sinusoids at several sample rates and the
`Data` arguments that go with them.  TEST INFRASTRUCTURE."""
import os

import numpy as np

TARGET_SR = 22050
HOP = 256
SENTENCES = ["the quick brown fox jumps over the lazy dog", "a short one", "she sells sea shells by the sea shore",
             "many years later he remembered that distant afternoon"]
DATA_KW = dict(filter_length=1024, hop_length=HOP, win_length=1024, sampling_rate=TARGET_SR, mel_fmin=0.0, mel_fmax=8000.0,
               max_wav_value=32768.0, p_arpabet=0.0, cmudict_path="", text_cleaners=[], randomize=False)


def grapheme_frontend(text):
    table = {c: i + 1 for i, c in enumerate("abcdefghijklmnopqrstuvwxyz '")}
    return [table[c] for c in text.lower() if c in table]


def write_wavs(root, rates, seconds=(0.31, 0.22, 0.27, 0.18), seed=0):
    """One wav per entry of `rates` -> the filelist rows [[path, sentence, speaker], ...] and every file's sample count."""
    from scipy.io.wavfile import write
    rs = np.random.RandomState(seed)
    rows, counts = [], []
    for i, sr in enumerate(rates):
        n = int(seconds[i % len(seconds)] * sr) + i               # odd lengths, no multiple of the hop
        t = np.arange(n) / sr
        y = sum(rs.uniform(0.2, 1.0) * np.sin(2 * np.pi * rs.uniform(80, 3000) * t + rs.uniform(0, 6.28)) for _ in range(5))
        path = os.path.join(str(root), "utt%02d_%d.wav" % (i, sr))
        write(path, sr, (0.9 * y / np.abs(y).max() * 32767.0).astype(np.int16))
        rows.append([path, SENTENCES[i % len(SENTENCES)], "0"])
        counts.append(n)
    return rows, counts
