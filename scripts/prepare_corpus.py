"""One pass over a filelist that writes the prepared corpus train.py then reads unchanged: every wav is brought to
--sampling-rate (audio_processing.resample_ragged), its leading and trailing silence is cut and its loudness brought to
--target-lufs (flowtron_amd.level.prepare), all on the device; the reference's data.py __main__ brought one step earlier.
The order is resample, then trim, then normalise: the trim and the loudness gate both look at levels in frames and blocks of the
final rate.  Written: DIR/<name>.wav (int16, mono), OUT (the filelist with the new paths and the same text and speaker columns)
and DIR/report.jsonl, one JSON line per file: path, source, orig_sampling_rate, start, end, n_out (samples at the final rate),
lufs_before (of the trimmed utterance), gain, peak_after.  Files are batched by rate and length; a batch costs one
device-to-host copy, which carries the audio and the report's numbers.
usage: python scripts/prepare_corpus.py --filelist IN --out-dir DIR --out-filelist OUT --sampling-rate 22050
           [--top-db 60 --target-lufs -23 --peak-ceiling 0.99 --max-gain-db 30 --frame-length 2048 --hop-length 512 --batch 64]"""
import argparse, json, os, sys, wave
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--filelist", required=True)
ap.add_argument("--out-dir", required=True)
ap.add_argument("--out-filelist", required=True)
ap.add_argument("--sampling-rate", type=int, required=True)
ap.add_argument("--top-db", type=float, default=60.0)
ap.add_argument("--target-lufs", type=float, default=-23.0)
ap.add_argument("--peak-ceiling", type=float, default=0.99)
ap.add_argument("--max-gain-db", type=float, default=30.0)
ap.add_argument("--frame-length", type=int, default=2048)
ap.add_argument("--hop-length", type=int, default=512)
ap.add_argument("--max-wav-value", type=float, default=32768.0)
ap.add_argument("--batch", type=int, default=64)
a = ap.parse_args()

import torch
from flowtron_amd import level
from flowtron_amd.audio import resample_ragged
from flowtron_amd.data import load_filepaths_and_text, load_wav_to_torch

rows = load_filepaths_and_text(a.filelist)
if not rows or any(len(r) < 1 or not r[0] for r in rows):
    sys.exit("%s: every line must start with a wav path" % a.filelist)
os.makedirs(a.out_dir, exist_ok=True)
names = [os.path.splitext(os.path.basename(r[0]))[0] + ".wav" for r in rows]
if len(set(names)) != len(names):
    sys.exit("%s: two files share a name; the output directory is flat" % a.filelist)

items = []                                        # (index, audio [n] fp32 in [-1, 1), its rate)
for i, r in enumerate(rows):
    x, sr = load_wav_to_torch(r[0])
    if x.dim() != 1:
        sys.exit("%s: mono only, got shape %s" % (r[0], tuple(x.shape)))
    items.append((i, x / a.max_wav_value, int(sr)))
items.sort(key=lambda it: (it[2], it[1].numel()))

report = [None] * len(rows)
for k in range(0, len(items), a.batch):
    group = items[k:k + a.batch]
    for sr in sorted({it[2] for it in group}):    # a batch holds one source rate
        part = [it for it in group if it[2] == sr]
        lens = [it[1].numel() for it in part]
        x = torch.zeros(len(part), max(lens))
        for b, it in enumerate(part):
            x[b, :lens[b]] = it[1]
        x = x.cuda()
        if sr != a.sampling_rate:
            x, n = resample_ragged(x, lens, sr, a.sampling_rate)
            lens = n.tolist()
        out, n_out, info = level.prepare(x, lens, a.sampling_rate, top_db=a.top_db, target_lufs=a.target_lufs, peak_ceiling=a.peak_ceiling,
                                         max_gain_db=a.max_gain_db, frame_length=a.frame_length, hop_length=a.hop_length)
        pcm = torch.round(torch.clamp(out, -1.0, 1.0) * 32767.0).to(torch.int16)
        nums = torch.stack([info.start.double(), info.end.double(), n_out.double(), info.lufs, info.gain.double(), info.peak.double()], 1)
        packed = torch.cat([pcm.view(torch.uint8).reshape(-1), nums.contiguous().view(torch.uint8).reshape(-1)]).cpu().numpy()   # the one copy
        pcm_h = packed[:pcm.numel() * 2].view("<i2").reshape(pcm.shape)
        nums_h = packed[pcm.numel() * 2:].view(np.float64).reshape(len(part), 6)
        for b, it in enumerate(part):
            start, end, n, lufs, gain, peak = nums_h[b]
            path = os.path.join(a.out_dir, names[it[0]])
            with wave.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(a.sampling_rate)
                w.writeframes(pcm_h[b, :int(n)].tobytes())
            report[it[0]] = dict(path=path, source=rows[it[0]][0], orig_sampling_rate=sr, start=int(start), end=int(end), n_out=int(n),
                                 lufs_before=None if not np.isfinite(lufs) else float(lufs), gain=float(gain), peak_after=float(gain * peak))

with open(a.out_filelist, "w", encoding="utf-8") as f:
    for r, j in zip(rows, report):
        f.write("|".join([j["path"]] + list(r[1:])) + "\n")
with open(os.path.join(a.out_dir, "report.jsonl"), "w", encoding="utf-8") as f:
    for j in report:
        f.write(json.dumps(j) + "\n")
print("%d files -> %s (%d Hz), filelist %s" % (len(rows), a.out_dir, a.sampling_rate, a.out_filelist))
